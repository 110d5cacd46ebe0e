// Stand-ins for the launchers of lr_refresh.hip (stub_touch.hpp says what a stand-in does): each counts its launch.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

std::atomic<unsigned long long> g_refresh_mask_launches{0}, g_refresh_share_launches{0}, g_refresh_recode_launches{0}, g_refresh_product_launches{0},
    g_refresh_lift_launches{0};

hipError_t launch_refresh_mask(const RefreshMaskLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_refresh_mask_launches.fetch_add(1);
    rd(L.lp, limbs);
    rd(L.mask, (long long)batch * L.words * L.n);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) wr(L.out + b * L.out_stride + (long long)i * L.n, L.n);
    return hipSuccess;
}

hipError_t launch_refresh_ckks_share(const RefreshCkksShareLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_refresh_share_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.mask + b * L.r_stride + row, L.n);
            rd(L.e1 + b * L.r_stride + row, L.n);
            rd(L.sk + b * L.sk_stride + row, L.n);
            rd(L.crs + b * L.crs_stride + row, L.n);
            wr(L.rec + b * L.rec_stride + row, L.n);
            if (i < L.dec_limbs) {
                rd(L.e0 + b * L.r_stride + row, L.n);
                rd(L.c1 + b * L.c1_stride + row, L.n);
                wr(L.dec + b * L.dec_stride + row, L.n);
            }
        }
    return hipSuccess;
}

hipError_t launch_refresh_recode(const RefreshRecodeLaunch &L, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, batch)) return verdict_error(v);
    g_refresh_recode_launches.fetch_add(1);
    rd(L.lp, L.limbs);
    rd(L.qmod, (long long)L.limbs * L.limbs);
    rd(L.ginv, L.limbs);
    rd(L.hdig, L.ls + 1);
    rd(L.qls, L.limbs);
    for (int b = 0; b < batch; ++b) {
        for (int i = 0; i <= L.ls; ++i) rd(L.in + b * L.in_stride + (long long)i * L.n, L.n);
        for (int i = L.row0; i < L.limbs; ++i) wr(L.out + b * L.out_stride + (long long)i * L.n, L.n);
    }
    return hipSuccess;
}

hipError_t launch_refresh_bfv_product(const RefreshBfvProductLaunch &L, int rows, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, rows, batch)) return verdict_error(v);
    g_refresh_product_launches.fetch_add(1);
    rd(L.lp, rows);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < rows; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.sk + b * L.sk_stride + row, L.n);
            if (i < L.nQ) wr(L.a + b * L.stride + row, L.n);
            wr(L.b + b * L.stride + row, L.n);
        }
    return hipSuccess;
}

hipError_t launch_refresh_bfv_lift(const RefreshBfvLiftLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_refresh_lift_launches.fetch_add(1);
    rd(L.lp, limbs);
    rd(L.delta_mont, limbs);
    rd(L.row, (long long)batch * L.n);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            wr(L.dec + b * L.dec_stride + row, L.n);
            if (L.rec) wr(L.rec + b * L.rec_stride + row, L.n);
            if (L.plus) rd(L.plus + b * L.plus_stride + row, L.n);
        }
    return hipSuccess;
}

}  // namespace lr
