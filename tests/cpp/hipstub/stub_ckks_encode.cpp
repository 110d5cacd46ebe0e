// Recording stand-ins for the launchers of lr_ckks_encode.hip (stub_touch.hpp says what a stand-in does): each counts its launch.
#include <atomic>

#include "lr_device.hpp"
#include "stub_touch.hpp"

namespace lr {

std::atomic<unsigned long long> g_ckks_stub_launches{0};
std::atomic<unsigned long long> g_ckks_stub_fused{0};      // fused Encode launches: only the fused route makes them
std::atomic<unsigned long long> g_ckks_stub_stages{0};     // streaming stages: only the tiled route makes them
namespace {
void tables(const CkksEncTables &tab) {
    rd(tab.roots, 2ll * tab.n + 1);
    rd(tab.rot, tab.n / 2);
}
void slots_r(const Cplx *v, int logslots, int batch) { rd(v, (long long)batch << logslots); }
void slots_w(Cplx *v, int logslots, int batch) { wr(v, (long long)batch << logslots); }
void plaintexts_w(const CkksScaleUp &S, int n, int batch) {
    rd(S.lp, S.limbs);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < S.limbs; ++i) wr(S.out + b * S.out_stride + (long long)i * n, n);
}
}  // namespace

hipError_t launch_ckks_encode_fused(const CkksEncTables &tab, const Cplx *values, int logslots, const CkksScaleUp &S, int batch, hipStream_t) {
    g_ckks_stub_launches.fetch_add(1);
    g_ckks_stub_fused.fetch_add(1);
    if (logslots < 0 || logslots > kCkksFusedMaxLogSlots || logslots > tab.logn - 1) return hipErrorInvalidValue;
    tables(tab);
    slots_r(values, logslots, batch);
    plaintexts_w(S, tab.n, batch);
    return hipSuccess;
}

hipError_t launch_ckks_dif_stage(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int loglen, int batch, hipStream_t) {
    g_ckks_stub_launches.fetch_add(1);
    g_ckks_stub_stages.fetch_add(1);
    if (loglen < 1 || loglen > logslots || logslots > tab.logn - 1) return hipErrorInvalidValue;
    tables(tab);
    slots_r(src, logslots, batch);
    slots_w(dst, logslots, batch);
    return hipSuccess;
}

hipError_t launch_ckks_dif_tile(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int logtile, int batch, hipStream_t) {
    g_ckks_stub_launches.fetch_add(1);
    if (logtile < 0 || logtile > logslots || logtile > kCkksFusedMaxLogSlots || logslots > tab.logn - 1) return hipErrorInvalidValue;
    tables(tab);
    slots_r(src, logslots, batch);
    slots_w(dst, logslots, batch);
    return hipSuccess;
}

hipError_t launch_ckks_scale_up(const CkksEncTables &tab, const Cplx *src, int logslots, const CkksScaleUp &S, int batch, hipStream_t) {
    g_ckks_stub_launches.fetch_add(1);
    if (logslots < 0 || logslots > tab.logn - 1) return hipErrorInvalidValue;
    slots_r(src, logslots, batch);
    plaintexts_w(S, tab.n, batch);
    return hipSuccess;
}

hipError_t launch_ckks_crt_to_double(const CkksEncTables &tab, const CkksCrt &P, int logslots, double *dbuf, int batch, hipStream_t) {
    g_ckks_stub_launches.fetch_add(1);
    if (logslots < 0 || logslots > tab.logn - 1 || P.words < 1 || P.words > kCkksCrtMaxWords || P.qhat_stride < P.words) return hipErrorInvalidValue;
    rd(P.lp, P.limbs);
    rd(P.inv, P.limbs);
    rd(P.Q, P.words);
    rd(P.Qhalf, P.words);
    for (int i = 0; i < P.limbs; ++i) rd(P.qhat + i * P.qhat_stride, P.words);
    for (int b = 0; b < batch; ++b)
        for (int i = 0; i < P.limbs; ++i) rd(P.pool + b * P.pool_stride + (long long)i * tab.n, tab.n);
    wr(dbuf, (long long)batch << (logslots + 1));
    return hipSuccess;
}

hipError_t launch_ckks_dit_tile(const CkksEncTables &tab, const double *dbuf, Cplx *dst, int logslots, int logtile, int batch, hipStream_t) {
    g_ckks_stub_launches.fetch_add(1);
    if (logtile < 0 || logtile > logslots || logtile > kCkksFusedMaxLogSlots || logslots > tab.logn - 1) return hipErrorInvalidValue;
    tables(tab);
    rd(dbuf, (long long)batch << (logslots + 1));
    slots_w(dst, logslots, batch);
    return hipSuccess;
}

hipError_t launch_ckks_dit_stage(const CkksEncTables &tab, const Cplx *src, Cplx *dst, int logslots, int loglen, int batch, hipStream_t) {
    g_ckks_stub_launches.fetch_add(1);
    g_ckks_stub_stages.fetch_add(1);
    if (loglen < 1 || loglen > logslots || logslots > tab.logn - 1) return hipErrorInvalidValue;
    tables(tab);
    slots_r(src, logslots, batch);
    slots_w(dst, logslots, batch);
    return hipSuccess;
}

}  // namespace lr
