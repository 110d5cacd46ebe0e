"""Worker of test_gpu_ckks_encryptor.py::test_device_form_replays_from_a_hip_graph (own process: torch brings its own HIP runtime and has
to initialise it before the library's).  After a warm-up call (the extender's pools at their size) lr_ckks_encryptor_encrypt_pk_device
enqueues kernels only, all on the one stream the contexts are set to, so torch.cuda.CUDAGraph can record and replay it."""
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
    nq, np_, B = len(Q), len(P), 2
    level = nq - 1
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    enc = ring.CkksEncryptor(cQ, cP, B)
    qp = lambda seed: ring.Poly(cQ, nq + np_, 1).set(sampling.uniform_poly(Q + P, N, 1, seed=seed))
    pk, pt = (qp(1), qp(2)), cQ.NewPoly(B).set(sampling.uniform_poly(Q, N, B, seed=3))
    rng = np.random.default_rng(4)
    bits = lambda: torch.from_numpy(rng.integers(0, 256, (B, N >> 3)).astype(np.uint8)).cuda()
    noise = lambda: torch.from_numpy((rng.integers(0, 20, (B, N)) | (rng.integers(0, 2, (B, N)) << 7)).astype(np.uint8)).cuda()
    uc, us, e0, e1 = bits(), bits(), noise(), noise()
    torch.cuda.synchronize()
    u_ptrs, e_ptrs = (uc.data_ptr(), us.data_ptr()), (e0.data_ptr(), e1.data_ptr())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cQ.SetStream(side.cuda_stream)
        cP.SetStream(side.cuda_stream)
        for fast in (False, True):
            out = (cQ.NewPoly(B), cQ.NewPoly(B))
            enc.EncryptPkDevice(pk, u_ptrs, e_ptrs, pt, out, level, fast=fast)    # warm-up outside the capture; its result is the reference
            side.synchronize()
            want = [p.get().copy() for p in out]
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                enc.EncryptPkDevice(pk, u_ptrs, e_ptrs, pt, out, level, fast=fast)
            for rep in range(2):
                for p in out:
                    p.set(np.zeros_like(want[0]))
                side.synchronize()
                graph.replay()
                side.synchronize()
                for k in range(2):
                    assert np.array_equal(out[k].get(), want[k]), (fast, rep, k)
            assert want[0].any() and want[1].any()
    print("graph replay ok")


if __name__ == "__main__":
    main()
