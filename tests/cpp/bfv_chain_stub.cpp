// Stand-in for launch_bfv_chain_step (lr_ewise.hip), for the CPU-sanitizer build of the BFV rotation chains' host side
// (tests/test_host_bfv_chain_sanitizers.py); every other launcher the chains reach is served by hipstub/stub_launch.cpp, which stays as it
// is.  TEST INFRASTRUCTURE: no arithmetic of the hot path lives here.  The stub asks the product's launch_verdict, counts its launch and
// touches the first and the last word of every row the real kernel would read or write: "device" memory is malloc'ed at its exact size, so
// a wrong pool size, stride or pool pair in the host code is an AddressSanitizer report.  It also checks what the pass relies on: an output
// is never the OTHER component's operand, and the next key-switch input is none of the operands.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

extern std::atomic<unsigned long long> g_stub_launches;
std::atomic<unsigned long long> g_bfv_chain_step_launches{0}, g_bfv_chain_step_last{0}, g_bfv_chain_step_crossed{0};

hipError_t launch_bfv_chain_step(const BfvChainStepLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_stub_launches.fetch_add(1);
    g_bfv_chain_step_launches.fetch_add(1);
    if (!L.cx_next) g_bfv_chain_step_last.fetch_add(1);
    if (L.out0 == L.a1 || L.out0 == L.p1 || L.out1 == L.a0 || L.out1 == L.p0 || L.p0 == L.a0 || L.p1 == L.a1 ||
        (L.cx_next && (L.cx_next == L.a0 || L.cx_next == L.a1 || L.cx_next == L.p0 || L.cx_next == L.p1 || L.cx_next == L.out0 || L.cx_next == L.out1)))
        g_bfv_chain_step_crossed.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.a0 + b * L.a0_stride + row, L.n);
            rd(L.p0 + b * L.p_stride + row, L.n);
            rd(L.p1 + b * L.p_stride + row, L.n);
            if (L.accumulate) rd(L.a1 + b * L.a1_stride + row, L.n);
            wr(L.out0 + b * L.out0_stride + row, L.n);
            wr(L.out1 + b * L.out1_stride + row, L.n);
            if (L.cx_next) wr(L.cx_next + b * L.cx_stride + row, L.n);
        }
    return hipSuccess;
}

}  // namespace lr
