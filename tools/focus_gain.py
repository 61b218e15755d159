#!/usr/bin/env python3
"""What the focus window buys chains that cross their best slabs.  W chains run as processes on ONE GPU over
the host shared-memory transport; every chain starts from the same adaptive seed of BASELINE config 2's input, and after every
epoch the chains exchange with cross-all.  Arm "focus": before every epoch chain r takes slice r of W of the file
(multi_gpu.focus_chain, --focus rank of the CLI).  Arm "plain": no window.  Both arms spend the same number of successful
evaluations per chain and epoch (to within one step), over the same chain seeds.  Prints per arm the mean best size after each
exchange and the mean number of regions the child took from each parent (mgl_cross_stats.regions_from).

    python tools/focus_gain.py [--chains 2,4] [--seeds 3] [--epochs 6] [--evals N] [--neighbours 4096] [--size 100000]"""
import argparse
import multiprocessing as mp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def chain(rank, world, path, nonce, data, seed, K, epochs, evals, focus, out):
    sys.path.insert(0, ROOT)
    os.environ.setdefault("MGL_COMM_TIMEOUT_S", "120")
    from megalania_amd import binding, multi_gpu

    comm = binding.Comm.shm(path, nonce, rank, world, 0)
    sa = binding.SA(data, neighbours_per_step=K, seed=multi_gpu.chain_seed(seed, rank), iters_per_epoch=len(data))
    sa.seed_adaptive()
    slab, cost = sa.current()
    sa.set_best(slab, cost)
    rows = []
    for e in range(epochs):
        if focus:
            multi_gpu.focus_chain(sa, rank, world, e)
        sa.begin_epoch(1, from_best=True)
        done = steps = 0
        while done < evals:
            st = sa.run(max(1, (evals - done) // K))  # a step yields at most K evaluations: only the last step can overshoot
            done += st["evaluations"]
            steps += st["steps"]
            if st["evaluations"] == 0:
                break
        own = sa.best()[1]
        xs = multi_gpu.exchange_cross_all_native(sa, comm, 64)
        x = xs["cross"]
        rows.append(dict(evals=done, steps=steps, own=own, best=sa.best()[1], distinct=xs["distinct"], parents=x["parents"],
                         regions=[int(r) for r in x["regions_from"][: xs["distinct"]]], adopted=x["adopted"]))
    sa.close()
    comm.close()
    out.put((rank, cost, rows))


def run_world(world, data, seed, K, epochs, evals, focus, tag):
    path = ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp") + "/mgl_focus_gain_%d_%s" % (os.getpid(), tag)
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=chain, args=(r, world, path, 0xF0C0 + world, data, seed, K, epochs, evals, focus, out)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r, (c, rows)) for r, c, rows in (out.get(timeout=900) for _ in procs))
    for p in procs:
        p.join(120)
        if p.exitcode != 0:
            raise SystemExit("a chain ended with exit code %r" % p.exitcode)
    return [res[r] for r in range(world)]


def size(cost):
    return 18 + cost / 16384.0  # 13 header bytes + 5 flush bytes, 16384 = 2048 * 8 cost units per byte


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="2,4")
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--evals", type=int, default=0, help="successful evaluations per chain and epoch (0 = the input's size)")
    ap.add_argument("--neighbours", type=int, default=4096)
    ap.add_argument("--size", type=int, default=100000)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from megalania_amd import corpus

    data, what = corpus.config_input("c2", a.size)
    evals = a.evals or len(data)
    print(f"input: {what}, {len(data)} bytes; K {a.neighbours}; {a.epochs} epochs of {evals} successful evaluations per chain; {a.seeds} seeds", flush=True)
    for world in (int(w) for w in a.chains.split(",")):
        for focus in (True, False):
            arm = "focus" if focus else "plain"
            after = [[] for _ in range(a.epochs)]    # per epoch: the common best size behind the exchange, one per seed
            own = [[] for _ in range(a.epochs)]      # per epoch: the chains' own best sizes in front of it
            regions = [[] for _ in range(world)]     # per parent index: regions the child took from it, one per crossing
            crossings = evals_seen = rows_seen = 0
            seed_size = None
            for s in range(a.seeds):
                res = run_world(world, data, 1673551 + 1000 * s, a.neighbours, a.epochs, evals, focus, f"{world}{arm}{s}")
                seed_size = size(res[0][0])
                for e in range(a.epochs):
                    rows = [res[r][1][e] for r in range(world)]
                    assert len({row["best"] for row in rows}) == 1, "cross-all leaves every chain the same cost"
                    after[e].append(size(rows[0]["best"]))
                    own[e] += [size(row["own"]) for row in rows]
                    evals_seen += sum(row["evals"] for row in rows)
                    rows_seen += len(rows)
                    if rows[0]["parents"]:
                        crossings += 1
                        for p, n in enumerate(rows[0]["regions"]):
                            regions[p].append(n)
            mean = lambda v: sum(v) / len(v) if v else float("nan")  # noqa: E731
            print(f"chains {world} arm {arm}: seed {seed_size:.1f} B; {evals_seen / rows_seen:.0f} evaluations per chain and epoch", flush=True)
            print("  best after exchange, mean B: " + " ".join(f"{mean(v):.1f}" for v in after), flush=True)
            print("  chains' own best before it, mean B: " + " ".join(f"{mean(v):.1f}" for v in own), flush=True)
            print(f"  crossings {crossings} of {a.seeds * a.epochs}; regions per parent, mean: " +
                  " ".join(f"{mean(v):.1f}" for v in regions if v), flush=True)


if __name__ == "__main__":
    main()
