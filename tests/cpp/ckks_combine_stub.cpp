// Recording stand-in for the launcher of lr_ckks_combine.hip, for the CPU-sanitizer build of lr_ckks_combine.cpp
// (tests/test_host_ckks_combine_sanitizers.py); the companion of hipstub/stub_launch.cpp, which stays as it is.  TEST INFRASTRUCTURE: no
// arithmetic of the hot path lives here.  The stub asks the product's launch_verdict, keeps a copy of the launch for the driver to read,
// and touches the first and the last word of every row the real kernel would read or write at the addresses the launch names: "device"
// memory is malloc'ed at its exact size, so a wrong stride, level, degree or batch in the host code is an AddressSanitizer report.
#include <atomic>
#include <mutex>
#include <vector>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

std::atomic<unsigned long long> g_combine_launches{0};
struct CombineRecord {
    CombineLaunch L;
    int limbs, batch;
};
std::mutex g_combine_mu;
std::vector<CombineRecord> g_combine_log;

hipError_t launch_ckks_combine(const CombineLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_combine_launches.fetch_add(1);
    rd(L.lp, limbs);
    const int comps = combine_comps(L.deg_a, L.deg_b);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            for (int u = 0; u < comps; ++u) {
                if (u <= L.deg_a) rd(L.a[u] + b * L.a_stride[u] + row, L.n);
                if (u <= L.deg_b) rd(L.b[u] + b * L.b_stride[u] + row, L.n);
                wr(L.out[u] + b * L.out_stride[u] + row, L.n);
            }
        }
    std::lock_guard<std::mutex> lock(g_combine_mu);
    g_combine_log.push_back(CombineRecord{L, limbs, batch});
    return hipSuccess;
}

}  // namespace lr
