"""Worker of test_gpu_collective.py::test_device_form_replays_from_a_hip_graph (own process: torch brings its own HIP runtime and has to
initialise it before the library's).  The _device share calls and the fold enqueue kernels only, all on the one stream the contexts are
set to, so torch.cuda.CUDAGraph can record and replay a CKS share, a PCKS share and the fold that follows them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def main():
    torch.cuda.init()
    pkg = graft.load_package()
    ring, params, sampling = pkg.ring, pkg.params, pkg.sampling
    N, Q, P = params.ckks_moduli("PN12QP109")
    Q, P = list(Q), list(P)
    rows, B, level = len(Q) + len(P), 3, len(Q) - 1
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    col = ring.Collective(cQ, cP, B)
    keys = [ring.Poly(cQ, rows, 1).set(sampling.uniform_poly(Q + P, N, 1, seed=s)) for s in (1, 2, 3, 4)]
    c0 = cQ.NewPoly(B).set(sampling.uniform_poly(Q, N, B, seed=5))
    c1 = cQ.NewPoly(B).set(sampling.uniform_poly(Q, N, B, seed=6))
    rng = np.random.default_rng(4)
    noise = lambda: torch.from_numpy((rng.integers(0, 39, (B, N)) | (rng.integers(0, 2, (B, N)) << 7)).astype(np.uint8)).cuda()
    plane = lambda: torch.from_numpy(rng.integers(0, 256, (B, N >> 3)).astype(np.uint8)).cuda()
    e, e0, e1, uc, us = noise(), noise(), noise(), plane(), plane()
    fill = sampling.uniform_poly(Q, N, B, seed=7)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cQ.SetStream(side.cuda_stream)
        cP.SetStream(side.cuda_stream)
        outs = [cQ.NewPoly(B) for _ in range(4)]

        def work():
            col.CkksCksShareDevice(keys[0], keys[1], c1, e.data_ptr(), outs[0], level)
            col.CkksPcksShareDevice(keys[0], (keys[2], keys[3]), c1, (uc.data_ptr(), us.data_ptr()), (e0.data_ptr(), e1.data_ptr()),
                                    (outs[1], outs[2]), level)
            col.Aggregate([outs[0], outs[1]], outs[3], level, base=c0)
        work()                                                           # warm-up outside the capture; its result is the reference
        side.synchronize()
        want = [o.get().copy() for o in outs]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            work()
        for rep in range(2):
            for o in outs:
                o.set(fill)
            side.synchronize()
            graph.replay()
            side.synchronize()
            for i, o in enumerate(outs):
                assert np.array_equal(o.get(), want[i]), (rep, i)
        assert all(not np.array_equal(w, fill) for w in want) and not np.array_equal(want[0], want[1])
    print("graph replay ok")


if __name__ == "__main__":
    main()
