"""Worker of test_gpu_refresh.py::test_device_form_replays_from_a_hip_graph (own process: torch brings its own HIP runtime and has to
initialise it before the library's).  The _device share call, the fold and the finalize enqueue kernels only, all on the one stream the
context is set to, so torch.cuda.CUDAGraph can record and replay a CKKS GenShares, Aggregate and Finalize."""
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
    N, Q, _ = params.ckks_moduli("PN12QP109")
    Q = list(Q)
    B, ls = 3, 0
    cQ = ring.NewContextWithParams(N, Q)
    r = ring.Refresh(cQ, None, 0, B)
    W = r.MaskWords(ls)
    sk = cQ.NewPoly(1).set(sampling.uniform_poly(Q, N, 1, seed=1))
    c0 = cQ.NewPoly(B).set(sampling.uniform_poly(Q, N, B, seed=5))
    c1 = cQ.NewPoly(B).set(sampling.uniform_poly(Q, N, B, seed=6))
    crs = cQ.NewPoly(B).set(sampling.uniform_poly(Q, N, B, seed=8))
    rng = np.random.default_rng(4)
    noise = lambda: torch.from_numpy((rng.integers(0, 20, (B, N)) | (rng.integers(0, 2, (B, N)) << 7)).astype(np.uint8)).cuda()
    bound = Q[0] // 6
    masks = [[int(rng.integers(0, bound)) - (bound >> 1) for _ in range(N)] for _ in range(B)]
    mask = torch.from_numpy(sampling.mask_word_planes(masks, W).view(np.int64)).cuda()
    e0, e1 = noise(), noise()
    fill = sampling.uniform_poly(Q, N, B, seed=7)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cQ.SetStream(side.cuda_stream)
        outs = [cQ.NewPoly(B) for _ in range(4)]

        def work():
            r.CkksGenSharesDevice(sk, ls, c1, crs, mask.data_ptr(), (e0.data_ptr(), e1.data_ptr()), (outs[0], outs[1]))
            r.Aggregate([outs[1], outs[1]], outs[2], len(Q) - 1)
            r.CkksFinalize(ls, c0, (outs[0], outs[2]), outs[3])
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
                got = o.get()
                rows = ls + 1 if i == 0 else len(Q)                      # limbs above levelStart of the decryption share keep the fill
                assert np.array_equal(got[:, :rows], want[i][:, :rows]), (rep, i)
        assert all(not np.array_equal(w, fill) for w in want[1:]) and not np.array_equal(want[1], want[3])
    print("graph replay ok")


if __name__ == "__main__":
    main()
