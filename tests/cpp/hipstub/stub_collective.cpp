// Stand-ins for the launchers of lr_collective.hip (stub_touch.hpp says what a stand-in does): each counts its launch.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

std::atomic<unsigned long long> g_cks_share_launches{0}, g_pcks_addend_launches{0}, g_fold_launches{0};

hipError_t launch_cks_share(const CksShareLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_cks_share_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.c1 + b * L.c1_stride + row, L.n);
            rd(L.sk_in + b * L.sk_in_stride + row, L.n);
            rd(L.sk_out + b * L.sk_out_stride + row, L.n);
            if (L.e) rd(L.e + b * L.e_stride + row, L.n);
            wr(L.out + b * L.out_stride + row, L.n);
        }
    return hipSuccess;
}

hipError_t launch_pcks_addend(const PcksAddendLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_pcks_addend_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.c1 + b * L.c1_stride + row, L.n);
            rd(L.sk + b * L.sk_stride + row, L.n);
            wr(L.out0 + b * L.out0_stride + row, L.n);
        }
    return hipSuccess;
}

hipError_t launch_fold(const FoldLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_fold_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            for (int k = 0; k < L.count; ++k) rd(L.share[k].base + b * L.share[k].stride + row, L.n);
            if (L.base) rd(L.base + b * L.base_stride + row, L.n);
            wr(L.out + b * L.out_stride + row, L.n);
        }
    return hipSuccess;
}

}  // namespace lr
