// Stand-ins for the launchers of lr_keygen.hip (stub_touch.hpp says what a stand-in does): each counts its launch.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

std::atomic<unsigned long long> g_keygen_skin_launches{0}, g_keygen_finish_launches{0}, g_keygen_pk_launches{0};

hipError_t launch_keygen_skin(const KeygenSkInLaunch &L, int limbs, int keys, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs, keys)) return verdict_error(v);
    g_keygen_skin_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int k = 0; k < keys; ++k) {
        if (!(L.gen[k] & 1u) || L.gen[k] >= 2u * (u32)L.n) return hipErrorInvalidValue;
        for (int i = 0; i < limbs; ++i) {
            rd(L.sk + k * L.sk_stride + (long long)i * L.n, L.n);
            wr(L.out + k * L.out_stride + (long long)i * L.n, L.n);
        }
    }
    return hipSuccess;
}

hipError_t launch_keygen_powers(const KeygenPowersLaunch &L, int limbs, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, limbs)) return verdict_error(v);
    g_keygen_skin_launches.fetch_add(1);
    rd(L.lp, limbs);
    for (int i = 0; i < limbs; ++i) {
        rd(L.sk + (long long)i * L.n, L.n);
        for (int k = 0; k < L.keys; ++k) wr(L.out + k * L.out_stride + (long long)i * L.n, L.n);
    }
    return hipSuccess;
}

hipError_t launch_keygen_finish(const KeygenFinishLaunch &L, int rows, int keys, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, rows, keys)) return verdict_error(v);
    g_keygen_finish_launches.fetch_add(1);
    rd(L.lp, rows);
    for (int k = 0; k < keys; ++k)
        for (int d = 0; d < L.beta; ++d)
            for (int i = 0; i < rows; ++i) {
                const long long row = (long long)i * L.n;
                rd(L.e + (long long)(k * L.beta + d) * L.e_stride + row, L.n);
                rd(L.key[k].base + (long long)(2 * d + 1) * L.key[k].stride + row, L.n);
                rd(L.skout + k * L.skout_stride + row, L.n);
                if (i >= d * L.alpha && i < (d + 1) * L.alpha && i < L.nQ) rd(L.skin + k * L.skin_stride + row, L.n);
                wr(L.key[k].base + (long long)(2 * d) * L.key[k].stride + row, L.n);
            }
    return hipSuccess;
}

hipError_t launch_keygen_pk(const KeygenPkLaunch &L, int rows, int batch, hipStream_t) {
    if (const LaunchVerdict v = launch_verdict(L, rows, batch)) return verdict_error(v);
    g_keygen_pk_launches.fetch_add(1);
    rd(L.lp, rows);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < rows; ++i) {
            const long long row = (long long)i * L.n;
            rd(L.sk + b * L.sk_stride + row, L.n);
            rd(L.pk1 + b * L.pk1_stride + row, L.n);
            wr(L.pk0 + b * L.pk0_stride + row, L.n);
        }
    return hipSuccess;
}

}  // namespace lr
