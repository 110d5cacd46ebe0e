// Recording stand-in for the launcher of lr_ckks_basis.hip, for the CPU-sanitizer build of lr_ckks_basis.cpp
// (tests/test_host_ckks_basis_sanitizers.py); the companion of hipstub/stub_launch.cpp, which stays as it is.  TEST INFRASTRUCTURE: no
// arithmetic of the hot path lives here.  The stub asks the product's launch_verdict, counts the launch (also as one of the launches the
// drivers' REFUSED macro watches) and its products, and touches the first and the last word of every row and of every table entry the
// real kernel would read or write at the addresses the launch names: "device" memory is malloc'ed at its exact size, so a wrong stride,
// level, pool, table offset or batch in the host code is an AddressSanitizer report.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

extern std::atomic<unsigned long long> g_stub_launches;      // hipstub/stub_launch.cpp
std::atomic<unsigned long long> g_ckks_basis_tail_launches{0}, g_ckks_basis_tail_products{0};

hipError_t launch_ckks_basis_tail(const BasisTailLaunch &L, int limbs, int products, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, products)) return verdict_error(v);
    g_stub_launches.fetch_add(1);
    g_ckks_basis_tail_launches.fetch_add(1);
    g_ckks_basis_tail_products.fetch_add((unsigned long long)products);
    rd(L.lp, limbs);
    const long long members = (long long)products * L.batch;
    for (int k = 0; k < products; ++k) {
        rd(L.products + k, 1);
        const BasisTailProduct P = L.products[k];
        rd(L.mult + (long long)k * L.row, limbs);
        rd(L.add + (long long)k * L.row, limbs);
        for (int u = 0; u < 2; ++u)
            for (int b = 0; b < L.batch; ++b)
                for (int i = 0; i < limbs; ++i) {
                    const long long row = (long long)i * L.n;
                    rd(L.stage + (u * members + (long long)k * L.batch + b) * L.stage_stride + row, L.n);
                    if (P.tail == 1) rd(L.c1[u] + b * L.c1_stride[u] + row, L.n);
                    wr(P.out[u] + b * P.out_stride + row, L.n);
                }
    }
    return hipSuccess;
}

}  // namespace lr
