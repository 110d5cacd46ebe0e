// Recording stand-ins for the launchers of lr_bfv_encode.hip (stub_touch.hpp says what a stand-in does): each counts its launch.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

std::atomic<unsigned long long> g_encoder_stub_launches{0};
std::atomic<unsigned long long> g_encoder_stub_fused{0};
namespace {
void tables(const EncoderTables &tab) { rd(tab.index, tab.n); }
void values_r(const void *values, long long n_values, int batch) {
    for (int b = 0; b < batch; ++b) rd((const u64 *)values + (long long)b * n_values, n_values);
}
void plaintexts_w(u64 *out, long long stride, int limbs, int n, const LimbParams *lp, const u64 *delta, int batch) {
    rd(lp, limbs);
    rd(delta, limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < limbs; ++i) wr(out + b * stride + (long long)i * n, n);
}
}  // namespace

hipError_t launch_bfv_encode_fused(const EncodeLaunch &L, int batch, hipStream_t) {
    g_encoder_stub_launches.fetch_add(1);
    g_encoder_stub_fused.fetch_add(1);
    if (L.tab.logn < 11 || L.tab.logn > 15 || L.tab.t >= (1ull << 31)) return hipErrorInvalidValue;
    tables(L.tab);
    rd(L.tw_inv, L.tab.n);
    values_r(L.values, L.n_values, batch);
    plaintexts_w(L.out, L.out_stride, L.limbs, L.tab.n, L.lp, L.delta_mont, batch);
    return hipSuccess;
}

hipError_t launch_bfv_decode_fused(const DecodeLaunch &L, int batch, hipStream_t) {
    g_encoder_stub_launches.fetch_add(1);
    g_encoder_stub_fused.fetch_add(1);
    if (L.tab.logn < 11 || L.tab.logn > 15 || L.tab.t >= (1ull << 31)) return hipErrorInvalidValue;
    tables(L.tab);
    rd(L.tw_fwd, L.tab.n);
    for (int b = 0; b < batch; ++b) {
        rd(L.in + (long long)b * L.tab.n, L.tab.n);
        wr((u64 *)L.values + (long long)b * L.tab.n, L.tab.n);
    }
    return hipSuccess;
}

hipError_t launch_bfv_slot_scatter(const EncoderTables &tab, const void *values, long long n_values, int, u64 *row, int batch, hipStream_t) {
    g_encoder_stub_launches.fetch_add(1);
    tables(tab);
    values_r(values, n_values, batch);
    for (int b = 0; b < batch; ++b) wr(row + (long long)b * tab.n, tab.n);
    return hipSuccess;
}

hipError_t launch_bfv_lift(const u64 *row, int n, u64 *out, long long out_stride, int limbs, const LimbParams *lp, const u64 *delta_mont, int batch,
                           hipStream_t) {
    g_encoder_stub_launches.fetch_add(1);
    for (int b = 0; b < batch; ++b) rd(row + (long long)b * n, n);
    plaintexts_w(out, out_stride, limbs, n, lp, delta_mont, batch);
    return hipSuccess;
}

hipError_t launch_bfv_slot_gather(const EncoderTables &tab, const u64 *row, void *values, int, int batch, hipStream_t) {
    g_encoder_stub_launches.fetch_add(1);
    tables(tab);
    for (int b = 0; b < batch; ++b) {
        rd(row + (long long)b * tab.n, tab.n);
        wr((u64 *)values + (long long)b * tab.n, tab.n);
    }
    return hipSuccess;
}

}  // namespace lr
