"""What do the row optimizer launches cost on one table?  ops.sparse_update_multi, "adam" and "sgd" (N unique rows of
a packed fp32 [R, 16] table, every launch on a different row set so that no row is cache-resident) and the
full-table flush ops.adam_catchup_all, each as launches serialised in one hipGraph between one pair of HIP events
(what the training step does).  Prints the median of REPS replays per launch, then every replay.
usage: python scripts/rowopt_probe.py [R] [N]"""
import sys

import numpy as np
import torch

from fuxictr_amd import _lib, ops

DEV = "cuda:0"
R = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 21
N = int(sys.argv[2]) if len(sys.argv) > 2 else 100000
D, SETS, STEP, REPS = 16, 8, 320, 7


class DD(object):
    pass


def timed_replays(build, before=None):
    """us per replay of the graph that `build` records, REPS times (`before` runs ahead of each, untimed)."""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        build()                                   # warm
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            build()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(REPS + 1):
        if before is not None:
            before()
        torch.cuda.synchronize()
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out[1:]                                # (the first replay uploads the graph)


def main():
    g = torch.Generator(device=DEV).manual_seed(1)
    table = torch.randn(R, D, device=DEV, generator=g)
    m = torch.randn(R, D, device=DEV, generator=g) * 1e-3
    v = torch.rand(R, D, device=DEV, generator=g) * 1e-6 + 1e-10
    last = torch.zeros(R, dtype=torch.int32, device=DEV)
    m0, v0 = m.clone(), v.clone()
    scal = ops.new_scalars(DEV, series=True)
    scal.view(torch.int32)[_lib.SC_STEP] = STEP - 1
    ops.opt_begin_step(scal)
    rng = np.random.default_rng(0)
    dds = []
    for _ in range(SETS):
        dd = DD()
        rows = np.sort(rng.choice(R, N, replace=False)).astype(np.int64)
        dd.uniq_row = torch.from_numpy(rows).to(DEV).to(torch.int32)
        dd.n_unique = torch.tensor([N], dtype=torch.int32, device=DEV)
        dd.n_max = N
        dds.append(dd)
    G = torch.randn(N, D, device=DEV, generator=g) * 1e-2
    gaps = torch.from_numpy(np.minimum((300 * rng.random(R) ** 3).astype(np.int64) + 1, 300)).to(DEV)
    stale = (STEP - gaps).to(torch.int32)         # gaps as in an aged run: 1 .. 300, power-law

    state = ops.RowState(table, m, v, last, D, G=G)
    sgd_state = ops.RowState(table, None, None, last, D, G=G)

    def adam():
        for dd in dds:
            ops.sparse_update_multi("adam", [state], dd, scal)

    def sgd():
        for dd in dds:
            ops.sparse_update_multi("sgd", [sgd_state], dd, scal)

    def flush():
        ops.adam_catchup_all(state, R, 0, scal)

    def age():                                    # (a flush decays the moments: every replay sees the same rows)
        last.copy_(stale)
        m.copy_(m0)
        v.copy_(v0)

    for name, fn, per, before in (("sparse_adam", adam, SETS, None), ("sparse_sgd", sgd, SETS, None),
                                  ("flush", flush, 1, age)):
        us = [t / per for t in timed_replays(fn, before)]
        print("%-12s median %8.2f us per launch   [%s]   R = %d, N = %d"
              % (name, float(np.median(us)), " ".join("%.2f" % t for t in us), R, N), flush=True)


if __name__ == "__main__":
    main()
