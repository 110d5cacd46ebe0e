// Stand-in for launch_bfv_relin_fold (lr_ewise.hip), for the CPU-sanitizer build of lr_bfv_relinearize_deg's host side
// (tests/test_host_bfv_relin_deg_sanitizers.py); every other launcher the call reaches is served by hipstub/stub_launch.cpp, which stays as
// it is.  TEST INFRASTRUCTURE: no arithmetic of the hot path lives here.  The stub asks the product's launch_verdict, counts its launch and
// its terms, and touches the first and the last word of every row the real kernel would read or write: "device" memory is malloc'ed at its
// exact size, so a wrong pool size, stride or group distance in the host code is an AddressSanitizer report.  It also checks what the pass
// relies on: an output is neither the other component's operand nor any term.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

extern std::atomic<unsigned long long> g_stub_launches;
std::atomic<unsigned long long> g_bfv_relin_fold_launches{0}, g_bfv_relin_fold_terms{0}, g_bfv_relin_fold_crossed{0};

hipError_t launch_bfv_relin_fold(const BfvRelinFoldLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_stub_launches.fetch_add(1);
    g_bfv_relin_fold_launches.fetch_add(1);
    g_bfv_relin_fold_terms.fetch_add((unsigned long long)L.terms);
    if (L.out[0] == L.p[0] || L.out[0] == L.p[1] || L.out[1] == L.p[0] || L.out[1] == L.p[1] || L.base[0] == L.p[0] || L.base[1] == L.p[1])
        g_bfv_relin_fold_crossed.fetch_add(1);
    rd(L.lp, limbs);
    for (int k = 0; k < 2; ++k)
        for (int b = 0; b < batch; ++b)
            for (int i = 0; i < limbs; ++i) {
                const long long row = (long long)i * L.n;
                rd(L.base[k] + b * L.base_stride[k] + row, L.n);
                for (int t = 0; t < L.terms; ++t) rd(L.p[k] + t * L.group_stride + b * L.p_stride + row, L.n);
                wr(L.out[k] + b * L.out_stride[k] + row, L.n);
            }
    return hipSuccess;
}

}  // namespace lr
