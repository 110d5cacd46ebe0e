"""Worker of test_gpu_keygen.py::test_device_form_replays_from_a_hip_graph (own process: torch brings its own HIP runtime and has to
initialise it before the library's).  lr_keygen_rotation_keys_device enqueues kernels only -- the keys' addresses and the Galois elements
travel in the kernel arguments -- all on the one stream the contexts are set to, so torch.cuda.CUDAGraph can record and replay it."""
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
    rows, K = len(Q) + len(P), 3
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    kg = ring.KeyGenerator(cQ, cP, K)
    beta, gens = kg.beta, [5, pow(5, -1, 2 * N), 2 * N - 1]
    sk = ring.Poly(cQ, rows, 1).set(sampling.uniform_poly(Q + P, N, 1, seed=1))
    a = sampling.uniform_poly(Q + P, N, 2 * beta, seed=2)
    rng = np.random.default_rng(4)
    e = torch.from_numpy((rng.integers(0, 20, (K, beta, N)) | (rng.integers(0, 2, (K, beta, N)) << 7)).astype(np.uint8)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cQ.SetStream(side.cuda_stream)
        cP.SetStream(side.cuda_stream)
        keys = [kg.NewSwitchingKey().set(a) for _ in range(K)]
        kg.GenRotationKeysDevice(sk, gens, e.data_ptr(), keys)       # warm-up outside the capture; its result is the reference
        side.synchronize()
        want = [k.get().copy() for k in keys]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            kg.GenRotationKeysDevice(sk, gens, e.data_ptr(), keys)
        for rep in range(2):
            for k in keys:
                k.set(a)
            side.synchronize()
            graph.replay()
            side.synchronize()
            for i in range(K):
                assert np.array_equal(keys[i].get(), want[i]), (rep, i)
        assert not np.array_equal(want[0][0::2], a[0::2]) and np.array_equal(want[0][1::2], a[1::2])
        assert not np.array_equal(want[0], want[1])
    print("graph replay ok")


if __name__ == "__main__":
    main()
