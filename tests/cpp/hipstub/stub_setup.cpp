// Stand-ins for the launchers of lr_setup.hip (stub_touch.hpp says what a stand-in does): each counts its launch.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

std::atomic<unsigned long long> g_setup_ckg_launches{0}, g_setup_share_launches{0}, g_setup_key_launches{0};

hipError_t launch_setup_ckg(const SetupCkgLaunch &L, int rows, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, rows, batch)) return verdict_error(v);
    g_setup_ckg_launches.fetch_add(1);
    rd(L.lp, rows);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < rows; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.sk + b * L.sk_stride + row, L.n);
            rd(L.crs + b * L.crs_stride + row, L.n);
            wr(L.share + b * L.share_stride + row, L.n);
        }
    return hipSuccess;
}

hipError_t launch_setup_share(int kind, const SetupShareLaunch &L, int rows, int parties, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, rows, parties)) return verdict_error(v);
    if (kind < kSetupRkg1 || kind > kSetupRtg) return hipErrorInvalidValue;
    g_setup_share_launches.fetch_add(1);
    rd(L.lp, rows);
    const bool pairs = kind == kSetupRkg2 || kind == kSetupNaive1 || kind == kSetupNaive2;
    const int per = pairs ? 2 : 1;
    for (int k = 0; k < parties; ++k) {
        if (kind == kSetupRtg && (!(L.gen[k] & 1u) || L.gen[k] >= 2u * (u32)L.n)) return hipErrorInvalidValue;
        for (int d = 0; d < L.beta; ++d)
            for (int i = 0; i < rows; ++i) {
                const long long row = (long long)i * L.n, z = (long long)k * L.beta + d;
                for (int c = 0; c < per; ++c) {
                    rd(L.e + (z * per + c) * L.e_stride + row, L.n);
                    wr(L.out[k].base + (long long)(per * d + c) * L.out[k].stride + row, L.n);
                }
                rd(L.sk + (kind == kSetupRtg ? 0 : k * L.sk_stride) + row, L.n);
                if (kind == kSetupRkg1 || kind == kSetupRkg3) rd(L.u + k * L.u_stride + row, L.n);
                if (kind == kSetupRkg1 || kind == kSetupRkg2 || kind == kSetupRtg) rd(L.crp + d * L.crp_stride + row, L.n);
                if (kind == kSetupRkg2) rd(L.in + d * L.in_stride + row, L.n);
                if (kind == kSetupRkg3) rd(L.in + (2 * d + 1) * L.in_stride + row, L.n);
                if (kind == kSetupNaive2) rd(L.in + 2 * d * L.in_stride + row, L.n), rd(L.in + (2 * d + 1) * L.in_stride + row, L.n);
                if (kind == kSetupNaive1 || kind == kSetupNaive2) {
                    rd(L.t + z * L.t_stride + row, L.n);
                    rd(L.pk0 + row, L.n);
                    rd(L.pk1 + row, L.n);
                }
            }
    }
    return hipSuccess;
}

hipError_t launch_setup_key(const SetupKeyLaunch &L, int rows, int beta, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, rows, beta)) return verdict_error(v);
    g_setup_key_launches.fetch_add(1);
    rd(L.lp, rows);
    for (int d = 0; d < beta; ++d)
        for (int i = 0; i < rows; ++i) {
            const long long row = (long long)i * L.n;
            if (L.pairs) rd(L.pairs + 2 * d * L.pairs_stride + row, L.n), rd(L.pairs + (2 * d + 1) * L.pairs_stride + row, L.n);
            if (L.polys) rd(L.polys + d * L.polys_stride + row, L.n);
            if (L.crp) rd(L.crp + d * L.crp_stride + row, L.n);
            wr(L.key + 2 * d * L.key_stride + row, L.n);
            wr(L.key + (2 * d + 1) * L.key_stride + row, L.n);
        }
    return hipSuccess;
}

}  // namespace lr
