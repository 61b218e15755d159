"""One chain of tests/test_gpu_cross_all.py: a process that joins the shared-memory communicator and runs the jobs it is given.
Kept apart from the test module, and free of imports at module level, so that a spawned process loads little."""
import os

K, SEED, STEPS = 64, 99, 20


def chain(rank, world, path, nonce, jobs, out):
    """jobs: one handle each -- data, slabs (per rank None or (PACKET bytes, cost)), grains (one exchange each, the best slab
    set anew before each), nomem_rank (that rank's first exchange finds no room), search (STEPS steps from the best slab at
    the end).  Puts (rank, per job the rows) on `out`."""
    os.environ["MGL_NO_AUTOBUILD"] = "1"
    os.environ["MGL_COMM_TIMEOUT_S"] = "60"  # a dead peer ends the exchange instead of hanging it
    import numpy as np
    from megalania_amd import binding, multi_gpu

    comm = binding.Comm.shm(path, nonce, rank, world, 0)
    res = []
    for job in jobs:
        mine = job["slabs"][rank]
        sa = binding.SA(job["data"], accept="single", neighbours_per_step=K, seed=multi_gpu.chain_seed(SEED, rank), iters_per_epoch=STEPS)
        rows = []
        for i, grain in enumerate(job["grains"]):
            if mine is not None:
                sa.set_best(np.frombuffer(mine[0], dtype=binding.PACKET), mine[1])
            if job.get("nomem_rank") == rank and i == 0:
                sa.debug_set(binding.KEY.CROSS_NOMEM, 1)  # this chain's next crossover finds no room for its buffers
            cur0, cur0_cost = sa.current()
            st = multi_gpu.exchange_cross_all_native(sa, comm, grain)
            best, cost = sa.best()
            cur1, cur1_cost = sa.current()
            rows.append(dict(st=st, best=best.tobytes(), cost=cost, hash=sa.slab_hash() if cost else None,
                             cur_same=bool((cur0 == cur1).all()) and cur0_cost == cur1_cost))
        if job.get("search"):
            sa.begin_epoch(1, from_best=True)  # what came from the peers is checked against the input here
            trace = [sa.run(1)["current_cost"] for _ in range(STEPS)]
            cur, cur_cost = sa.current()
            best, best_cost = sa.best()
            rows.append(dict(trace=trace, cur=cur.tobytes(), cur_cost=cur_cost, best=best.tobytes(), best_cost=best_cost))
        sa.close()
        res.append(rows)
    comm.close()
    out.put((rank, res))
