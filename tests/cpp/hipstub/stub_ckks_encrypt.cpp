// Stand-ins for the launchers of lr_ckks_encrypt.hip (stub_touch.hpp says what a stand-in does): each counts its launch.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

extern std::atomic<unsigned long long> g_encryptor_stub_launches;      // stub_bfv_encrypt.cpp
std::atomic<unsigned long long> g_ckks_expand_launches{0}, g_ckks_fast_launches{0};

hipError_t launch_ckks_expand(const CkksExpandLaunch &L, int limbs, int batch, hipStream_t) {
    const int parts = L.ternary + L.noises;
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_encryptor_stub_launches.fetch_add(1);
    g_ckks_expand_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b) {
        if (L.ternary) {
            rd(L.coeff_bits + (long long)b * (L.n >> 3), L.n >> 3);
            rd(L.sign_bits + (long long)b * (L.n >> 3), L.n >> 3);
        }
        for (int k = 0; k < L.noises; ++k) rd(L.e[k] + (long long)b * L.n, L.n);
        for (int p = 0; p < parts; ++p)
            for (int i = 0; i < limbs; ++i) wr(L.out + p * L.part_stride + b * L.out_stride + (long long)i * L.n, L.n);
    }
    return hipSuccess;
}

hipError_t launch_ckks_pk_fast(const CkksPkFastLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_encryptor_stub_launches.fetch_add(1);
    g_ckks_fast_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.u + b * L.r_stride + row, L.n);
            rd(L.e0 + b * L.r_stride + row, L.n);
            rd(L.e1 + b * L.r_stride + row, L.n);
            rd(L.pk0 + b * L.pk0_stride + row, L.n);
            rd(L.pk1 + b * L.pk1_stride + row, L.n);
            rd(L.pt + b * L.pt_stride + row, L.n);
            wr(L.out0 + b * L.out0_stride + row, L.n);
            wr(L.out1 + b * L.out1_stride + row, L.n);
        }
    return hipSuccess;
}

hipError_t launch_ckks_sk_fast(const CkksSkFastLaunch &L, int limbs, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, batch)) return verdict_error(v);
    g_encryptor_stub_launches.fetch_add(1);
    g_ckks_fast_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.crp + b * L.crp_stride + row, L.n);
            rd(L.sk + b * L.sk_stride + row, L.n);
            rd(L.e + b * L.e_stride + row, L.n);
            rd(L.pt + b * L.pt_stride + row, L.n);
            wr(L.out0 + b * L.out0_stride + row, L.n);
            wr(L.out1 + b * L.out1_stride + row, L.n);
        }
    return hipSuccess;
}

}  // namespace lr
