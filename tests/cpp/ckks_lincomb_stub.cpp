// Recording stand-in for the launcher of lr_ckks_lincomb.hip, for the CPU-sanitizer build of lr_ckks_lincomb.cpp
// (tests/test_host_ckks_lincomb_sanitizers.py); the companion of hipstub/stub_launch.cpp, which stays as it is.  TEST INFRASTRUCTURE: no
// arithmetic of the hot path lives here.  The stub asks the product's launch_verdict, keeps a copy of the launch for the driver to read,
// and touches the first and the last word of every row the real kernel would read or write at the addresses the launch names: "device"
// memory is malloc'ed at its exact size, so a wrong stride, level, limb range or term count in the host code is an AddressSanitizer report.
#include <atomic>
#include <mutex>
#include <vector>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

std::atomic<unsigned long long> g_lincomb_launches{0};
struct LinCombRecord {
    LinCombLaunch L;
    int limbs, batch;
};
std::mutex g_lincomb_mu;
std::vector<LinCombRecord> g_lincomb_log;

hipError_t launch_ckks_lincomb(const LinCombLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_lincomb_launches.fetch_add(1);
    rd(L.lp + L.limb0, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = L.limb0; i < L.limb0 + limbs; ++i) {
            const long long row = (long long)i * L.n;
            for (int u = 0; u < 2; ++u) {
                for (int k = 0; k < L.count; ++k) rd(L.term[k].c[u] + b * L.term[k].stride[u] + row, L.n);
                wr(L.out[u] + b * L.out_stride[u] + row, L.n);
            }
        }
    std::lock_guard<std::mutex> lock(g_lincomb_mu);
    g_lincomb_log.push_back(LinCombRecord{L, limbs, batch});
    return hipSuccess;
}

}  // namespace lr
