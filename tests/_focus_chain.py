"""One chain of tests/test_gpu_focus.py: a process that joins the shared-memory communicator, takes its slice of the file round
by round and crosses its best slab with the other chain's.  Kept apart from the test module, and free of imports at module
level, so that a spawned process loads little."""
import os

K, SEED, STEPS, ROUNDS = 64, 4711, 20, 2


def chain(rank, world, path, nonce, data, out):
    """Both chains seed the same greedy parse as their best slab.  Per round: the slice (multi_gpu.focus_chain), an epoch of
    STEPS steps from the best slab, exchange_cross_all.  Puts (rank, start slab, rows) on `out`; a row holds the window, the
    best slab and cost behind the search, and the best slab's cost and hash behind the exchange."""
    os.environ["MGL_NO_AUTOBUILD"] = "1"
    os.environ["MGL_COMM_TIMEOUT_S"] = "60"  # a dead peer ends the exchange instead of hanging it
    from megalania_amd import binding, multi_gpu

    comm = binding.Comm.shm(path, nonce, rank, world, 0)
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=multi_gpu.chain_seed(SEED, rank), iters_per_epoch=STEPS * K)
    sa.seed_greedy(8)
    start, start_cost = sa.current()
    sa.set_best(start, start_cost)
    rows = []
    for rnd in range(ROUNDS):
        lo, hi = multi_gpu.focus_chain(sa, rank, world, rnd)
        sa.begin_epoch(1, from_best=True)  # what came from the peer is checked against the input here
        epoch_start, epoch_cost = sa.current()
        st = sa.run(STEPS)
        searched, searched_cost = sa.best()
        xs = multi_gpu.exchange_cross_all_native(sa, comm, 64)
        best, cost = sa.best()
        rows.append(dict(window=(lo, hi), focus=sa.focus(), epoch_start=epoch_start.tobytes(), epoch_cost=epoch_cost, steps=st["steps"],
                         searched=searched.tobytes(), searched_cost=searched_cost, xs=xs, best=best.tobytes(), cost=cost, hash=sa.slab_hash()))
    sa.begin_epoch(1, from_best=True)
    rows.append(dict(final_cost=sa.current()[1]))
    sa.close()
    comm.close()
    out.put((rank, start.tobytes(), start_cost, rows))
