// Recording stand-in for the launcher of lr_ckks_chain.hip, for the CPU-sanitizer build of lr_ckks_chain.cpp
// (tests/test_host_ckks_chain_sanitizers.py); the companion of hipstub/stub_launch.cpp, which stays as it is.  TEST INFRASTRUCTURE: no
// arithmetic of the hot path lives here.  The stub asks the product's launch_verdict, counts the launch (also as one of the launches the
// drivers' REFUSED macro watches), and touches the first and the last word of every row the real kernel would read or write at the
// addresses the launch names: "device" memory is malloc'ed at its exact size, so a wrong stride, level, pool or batch in the host code
// is an AddressSanitizer report.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

extern std::atomic<unsigned long long> g_stub_launches;      // hipstub/stub_launch.cpp
std::atomic<unsigned long long> g_ckks_chain_step_launches{0};

hipError_t launch_ckks_chain_step(const CkksChainStepLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_stub_launches.fetch_add(1);
    g_ckks_chain_step_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.a0 + b * L.a0_stride + row, L.n);
            rd(L.a1 + b * L.a1_stride + row, L.n);
            wr(L.plus0 + b * L.plus_stride + row, L.n);
            wr(L.cx + b * L.cx_stride + row, L.n);
        }
    return hipSuccess;
}

}  // namespace lr
