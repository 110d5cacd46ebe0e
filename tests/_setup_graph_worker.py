"""Worker of test_gpu_setup.py::test_device_form_replays_from_a_hip_graph (own process: torch brings its own HIP runtime and has to
initialise it before the library's).  lr_setup_rkg_round1_device enqueues kernels only -- the shares' addresses travel in the kernel
arguments -- all on the one stream the contexts are set to, so torch.cuda.CUDAGraph can record and replay it (a single-stream capture)."""
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
    K = 3
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    st = ring.Setup(cQ, cP, K)
    beta = st.beta
    sk = st.NewPoly(K).set(sampling.uniform_poly(Q + P, N, K, seed=1))
    u = st.NewPoly(K).set(sampling.uniform_poly(Q + P, N, K, seed=2))
    crp = st.NewShare().set(sampling.uniform_poly(Q + P, N, beta, seed=3))
    pattern = sampling.uniform_poly(Q + P, N, beta, seed=5)
    rng = np.random.default_rng(4)
    e = torch.from_numpy((rng.integers(0, 20, (K, beta, N)) | (rng.integers(0, 2, (K, beta, N)) << 7)).astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cQ.SetStream(side.cuda_stream)
        cP.SetStream(side.cuda_stream)
        shares = [st.NewShare().set(pattern) for _ in range(K)]
        st.RkgRound1Device(u, sk, crp, e.data_ptr(), shares)       # warm-up outside the capture; its result is the reference
        side.synchronize()
        want = [s.get().copy() for s in shares]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st.RkgRound1Device(u, sk, crp, e.data_ptr(), shares)
        for rep in range(2):
            for s in shares:
                s.set(pattern)
            side.synchronize()
            graph.replay()
            side.synchronize()
            for i in range(K):
                assert np.array_equal(shares[i].get(), want[i]), (rep, i)
        assert not np.array_equal(want[0], pattern) and not np.array_equal(want[0], want[1])
    print("graph replay ok")


if __name__ == "__main__":
    main()
