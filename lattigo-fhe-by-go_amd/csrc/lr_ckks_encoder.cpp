// lr_ckks_encoder.cpp -- C ABI: lr_ckks_encoder, ckks.Encoder (ckks/encoder.go:31-226) for a batch of plaintexts on the device.
// The host sanitizer build (tests/host_stub_build.py) compiles this unit with every other; the launchers of lr_ckks_encode.hip have their
// stand-in in tests/cpp/hipstub/stub_ckks_encode.cpp.
#include "lr_host.hpp"

#include <cmath>

// what ckks.NewEncoder builds (ckks/encoder.go:31-69), the decoder's CRT tables, and the staging of the host-value entry points
struct lr_ckks_encoder {
    int device = 0;
    lr_context *cQ = nullptr;
    int max_batch = 0;
    bool tiled = false;                       // Options::ckks_encoder_tiled: the tiled route at every slot count
    std::vector<u64> rot_group;               // [m / 2], the upper half zero as in the reference
    std::vector<double> roots;                // [2 (m + 1)]
    HostCkksCrt crt;
    u32 *d_rot = nullptr;
    Cplx *d_roots = nullptr;
    u64 *d_qhat = nullptr, *d_inv = nullptr, *d_Q = nullptr, *d_Qhalf = nullptr;
    u64 *d_pool = nullptr;                    // polypool: [max_batch][|Q|][N], Decode's coefficient-domain image
    double *d_dbuf = nullptr;                 // [max_batch][N]: the used coefficients as doubles, real parts then imaginary parts
    Cplx *d_scratch = nullptr;                // [max_batch][N / 2]: the tiled route's slots between launches
    Cplx *d_values = nullptr;                 // the host-value entry points' slots on the device, [max_batch][N / 2]
    Cplx *h_values = nullptr;                 // the same, pinned
    hipEvent_t staged = nullptr;              // the last copy out of h_values: the next call waits for it before it refills the buffer
    ~lr_ckks_encoder() {
        for (void *p : {(void *)d_rot, (void *)d_roots, (void *)d_qhat, (void *)d_inv, (void *)d_Q, (void *)d_Qhalf, (void *)d_pool, (void *)d_dbuf,
                        (void *)d_scratch, (void *)d_values})
            if (p) (void)hipFree(p);
        if (h_values) (void)hipHostFree(h_values);
        if (staged) (void)hipEventDestroy(staged);
    }
};

namespace lr_host {
namespace {

// The route decision: the fused kernels hold 16 * slots bytes in one CU's LDS
bool ckks_encoder_fused(const lr_ckks_encoder *e, int logslots) { return !e->tiled && logslots <= kCkksFusedMaxLogSlots; }

CkksEncTables ckks_tables(const lr_ckks_encoder *e) {
    CkksEncTables tab;
    tab.roots = e->d_roots;
    tab.rot = e->d_rot;
    tab.n = (int)e->cQ->h.N;
    tab.logn = (int)e->cQ->h.logN;
    return tab;
}

// null handles, the poly against contextQ, the level and the batch against the poly and max_batch, the slot count, the scale
int ckks_encoder_check(const lr_ckks_encoder *e, const lr_poly *pt, int slots, int level, double scale, int batch, int *logslots) {
    if (!e || !pt) return fail(LR_ERR_ARG, "null argument");
    if (pt->ctx != e->cQ) return fail(LR_ERR_ARG, "CKKS encoder: the plaintext poly belongs to another context");
    if (slots < 1 || (slots & (slots - 1)) != 0 || (u64)slots > e->cQ->h.N / 2)
        return fail(LR_ERR_ARG, "CKKS encoder: slots must be a power of two between 1 and N/2 (ckks/encoder.go:84)");
    if (!(scale > 0) || !std::isfinite(scale)) return fail(LR_ERR_ARG, "CKKS encoder: the scale must be finite and positive");
    if (level < 0 || level >= e->cQ->h.L()) return fail(LR_ERR_SHAPE, "CKKS encoder: level outside 0 .. |Q| - 1");
    if (pt->N != e->cQ->h.N || pt->limbs < level + 1) return fail(LR_ERR_SHAPE, "CKKS encoder: the plaintext poly must hold level + 1 limbs");
    if (batch < 1 || batch != pt->batch) return fail(LR_ERR_SHAPE, "CKKS encoder: batch differs from the plaintext poly's");
    if (batch > e->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the encoder's max_batch");
    int l = 0;
    while ((1 << l) < slots) ++l;
    *logslots = l;
    return LR_OK;
}

// Encode (ckks/encoder.go:78-116) of slot values already on the device
int ckks_encode_on_device(lr_ckks_encoder *e, const Cplx *d_values, int logslots, int level, double scale, int batch, lr_poly *pt) {
    hipStream_t s = e->cQ->stream;
    const CkksEncTables tab = ckks_tables(e);
    CkksScaleUp S;
    S.out = pt->d;
    S.out_stride = pt->stride();
    S.limbs = level + 1;
    S.lp = e->cQ->d_lp;
    S.scale = scale;
    if (ckks_encoder_fused(e, logslots) && batch >= kCkksOneKernelBatch) {
        LR_HIP(launch_ckks_encode_fused(tab, d_values, logslots, S, batch, s));
    } else if (ckks_encoder_fused(e, logslots)) {
        // too few plaintexts for a workgroup each to fill the chip with the scale-up's stores: invfft in LDS, then the scale-up grid-wide
        LR_HIP(launch_ckks_dif_tile(tab, d_values, e->d_scratch, logslots, logslots, batch, s));
        LR_HIP(launch_ckks_scale_up(tab, e->d_scratch, logslots, S, batch, s));
    } else {
        // invfftlazy's stages above the tile stream over the scratch, the first of them out of the caller's values
        const int logtile = ckks_tile_log(logslots);
        const Cplx *src = d_values;
        for (int ll = logslots; ll > logtile; --ll) {
            LR_HIP(launch_ckks_dif_stage(tab, src, e->d_scratch, logslots, ll, batch, s));
            src = e->d_scratch;
        }
        LR_HIP(launch_ckks_dif_tile(tab, src, e->d_scratch, logslots, logtile, batch, s));
        LR_HIP(launch_ckks_scale_up(tab, e->d_scratch, logslots, S, batch, s));
    }
    const Rows rows = rows_of(pt);
    return run_ntt(e->cQ, false, rows, rows, 0, 1, level + 1, batch);                 // NTTLvl(level), :107
}

// Decode (ckks/encoder.go:119-168) into slot values on the device
int ckks_decode_on_device(lr_ckks_encoder *e, const lr_poly *pt, int logslots, int level, double scale, int batch, Cplx *d_values) {
    const HostContext &hQ = e->cQ->h;
    hipStream_t s = e->cQ->stream;
    const CkksEncTables tab = ckks_tables(e);
    const long long pool_stride = (long long)(level + 1) * (long long)hQ.N;
    LR_TRY(run_ntt(e->cQ, true, rows_of(pt), Rows{e->d_pool, pool_stride, 0, 1}, 0, 1, level + 1, batch));      // InvNTTLvl(level), :121
    const size_t L = (size_t)hQ.L();
    CkksCrt P;
    P.pool = e->d_pool;
    P.pool_stride = pool_stride;
    P.limbs = level + 1;
    P.words = e->crt.words[level];
    P.lp = e->cQ->d_lp;
    P.qhat = e->d_qhat + (size_t)level * L * e->crt.stride;
    P.qhat_stride = e->crt.stride;
    P.inv = e->d_inv + (size_t)level * L;
    P.Q = e->d_Q + (size_t)level * e->crt.stride;
    P.Qhalf = e->d_Qhalf + (size_t)level * e->crt.stride;
    P.scale = scale;
    LR_HIP(launch_ckks_crt_to_double(tab, P, logslots, e->d_dbuf, batch, s));
    if (ckks_encoder_fused(e, logslots)) {
        LR_HIP(launch_ckks_dit_tile(tab, e->d_dbuf, d_values, logslots, logslots, batch, s));
        return LR_OK;
    }
    // fft's stages up to the tile in LDS, the wider ones streaming over the scratch, the last of them into the caller's values
    const int logtile = ckks_tile_log(logslots);
    LR_HIP(launch_ckks_dit_tile(tab, e->d_dbuf, logtile == logslots ? d_values : e->d_scratch, logslots, logtile, batch, s));
    for (int ll = logtile + 1; ll <= logslots; ++ll)
        LR_HIP(launch_ckks_dit_stage(tab, e->d_scratch, ll == logslots ? d_values : e->d_scratch, logslots, ll, batch, s));
    return LR_OK;
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_ckks_encoder_create(lr_context *cQ, int max_batch, const double *roots, lr_ckks_encoder **out) {
    return lr_ckks_encoder_create_ex(cQ, max_batch, roots, nullptr, out);
}

extern "C" int lr_ckks_encoder_create_ex(lr_context *cQ, int max_batch, const double *roots, const lr_options *options, lr_ckks_encoder **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    Options parsed = cQ->opt;
    if (options) LR_TRY(options_from_public(options, &parsed));
    else parsed.apply_env();
    if (max_batch < 1 || max_batch > 65535) return fail(LR_ERR_ARG, "max_batch must be in 1 .. 65535");
    const HostContext &hQ = cQ->h;
    if (hQ.N < 2 || hQ.logN > 16) return fail(LR_ERR_ARG, "CKKS encoder: N must be in 2 .. 2^16");
    std::unique_ptr<lr_ckks_encoder> e(new lr_ckks_encoder());
    e->cQ = cQ;
    e->device = cQ->device;
    e->max_batch = max_batch;
    e->tiled = parsed.ckks_encoder_tiled;
    if (!build_ckks_crt(hQ, kCkksCrtMaxWords, e->crt)) return fail(LR_ERR_ARG, "CKKS encoder: Q exceeds 2048 bits, the limit of the decoder's multi-word CRT");
    const u64 N = hQ.N, m = 2 * N;
    e->rot_group.assign(m >> 1, 0);                                     // :39-45
    u64 five_pows = 1;
    for (u64 i = 0; i < (m >> 2); ++i) {
        e->rot_group[i] = five_pows;
        five_pows = (five_pows * 5) & (m - 1);                          // GaloisGen = 5
    }
    e->roots.resize(2 * (m + 1));
    if (roots) {
        std::copy(roots, roots + 2 * (m + 1), e->roots.begin());
    } else {
        for (u64 i = 0; i < m; ++i) {                                   // :47-53, with the host libm for Go's math.Cos / math.Sin
            const double angle = 2 * 3.141592653589793 * (double)i / (double)m;
            e->roots[2 * i] = std::cos(angle);
            e->roots[2 * i + 1] = std::sin(angle);
        }
        e->roots[2 * m] = e->roots[0];
        e->roots[2 * m + 1] = e->roots[1];
    }
    LR_HIP(hipSetDevice(cQ->device));
    std::vector<u32> rot32(e->rot_group.begin(), e->rot_group.begin() + (m >> 2));
    LR_TRY(to_device(&e->d_rot, rot32.data(), rot32.size()));
    LR_TRY(to_device(&e->d_roots, (const Cplx *)e->roots.data(), (size_t)(m + 1)));
    LR_TRY(to_device(&e->d_qhat, e->crt.qhat.data(), e->crt.qhat.size()));
    LR_TRY(to_device(&e->d_inv, e->crt.inv.data(), e->crt.inv.size()));
    LR_TRY(to_device(&e->d_Q, e->crt.Q.data(), e->crt.Q.size()));
    LR_TRY(to_device(&e->d_Qhalf, e->crt.Qhalf.data(), e->crt.Qhalf.size()));
    const size_t coeffs = (size_t)max_batch * N;                        // N doubles = N / 2 complex values per plaintext
    LR_HIP(hipMalloc((void **)&e->d_pool, coeffs * (size_t)hQ.L() * sizeof(u64)));
    LR_HIP(hipMalloc((void **)&e->d_dbuf, coeffs * sizeof(double)));
    LR_HIP(hipMalloc((void **)&e->d_scratch, coeffs * sizeof(double)));
    LR_HIP(hipMalloc((void **)&e->d_values, coeffs * sizeof(double)));
    LR_HIP(hipHostMalloc((void **)&e->h_values, coeffs * sizeof(double), 0));
    LR_HIP(hipEventCreateWithFlags(&e->staged, hipEventDisableTiming));
    *out = e.release();
    return LR_OK;
    });
}

extern "C" int lr_ckks_encoder_destroy(lr_ckks_encoder *e) {
    return guarded([&]() -> int {
    if (!e) return LR_OK;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its context's caller-supplied stream
    delete e;
    return LR_OK;
    });
}

extern "C" int lr_ckks_encoder_tables(const lr_ckks_encoder *e, uint64_t *rot_group, double *roots) {
    return guarded([&]() -> int {
    if (!e || !rot_group || !roots) return fail(LR_ERR_ARG, "null argument");
    std::copy(e->rot_group.begin(), e->rot_group.end(), rot_group);
    std::copy(e->roots.begin(), e->roots.end(), roots);
    return LR_OK;
    });
}

extern "C" int lr_ckks_encoder_route(const lr_ckks_encoder *e, int slots, int *fused) {
    return guarded([&]() -> int {
    if (!e || !fused) return fail(LR_ERR_ARG, "null argument");
    if (slots < 1 || (slots & (slots - 1)) != 0 || (u64)slots > e->cQ->h.N / 2)
        return fail(LR_ERR_ARG, "CKKS encoder: slots must be a power of two between 1 and N/2 (ckks/encoder.go:84)");
    int logslots = 0;
    while ((1 << logslots) < slots) ++logslots;
    *fused = ckks_encoder_fused(e, logslots) ? 1 : 0;
    return LR_OK;
    });
}

extern "C" int lr_ckks_encode(lr_ckks_encoder *e, const double *values, int slots, int level, double scale, int batch, lr_poly *pt) {
    return guarded([&]() -> int {
    int logslots = 0;
    LR_TRY(ckks_encoder_check(e, pt, slots, level, scale, batch, &logslots));
    if (!values) return fail(LR_ERR_ARG, "null argument");
    LR_HIP(hipSetDevice(e->device));
    // the caller's slots through the pinned buffer to the device; the caller's array is free on return
    const size_t bytes = (size_t)batch * (size_t)slots * sizeof(Cplx);
    LR_HIP(hipEventSynchronize(e->staged));               // the copy of the call before has left the pinned buffer
    std::memcpy(e->h_values, values, bytes);
    LR_HIP(hipMemcpyAsync(e->d_values, e->h_values, bytes, hipMemcpyHostToDevice, e->cQ->stream));
    LR_HIP(hipEventRecord(e->staged, e->cQ->stream));
    return ckks_encode_on_device(e, e->d_values, logslots, level, scale, batch, pt);
    });
}

extern "C" int lr_ckks_decode(lr_ckks_encoder *e, const lr_poly *pt, int slots, int level, double scale, int batch, double *values) {
    return guarded([&]() -> int {
    int logslots = 0;
    LR_TRY(ckks_encoder_check(e, pt, slots, level, scale, batch, &logslots));
    if (!values) return fail(LR_ERR_ARG, "null argument");
    LR_HIP(hipSetDevice(e->device));
    LR_TRY(ckks_decode_on_device(e, pt, logslots, level, scale, batch, e->d_values));
    const size_t bytes = (size_t)batch * (size_t)slots * sizeof(Cplx);
    LR_HIP(hipEventSynchronize(e->staged));
    LR_HIP(hipMemcpyAsync(e->h_values, e->d_values, bytes, hipMemcpyDeviceToHost, e->cQ->stream));
    LR_HIP(hipStreamSynchronize(e->cQ->stream));
    std::memcpy(values, e->h_values, bytes);
    return LR_OK;
    });
}

extern "C" int lr_ckks_encode_device(lr_ckks_encoder *e, const void *device_values, int slots, int level, double scale, int batch, lr_poly *pt) {
    return guarded([&]() -> int {
    int logslots = 0;
    LR_TRY(ckks_encoder_check(e, pt, slots, level, scale, batch, &logslots));
    if (!device_values) return fail(LR_ERR_ARG, "null argument");
    LR_HIP(hipSetDevice(e->device));
    return ckks_encode_on_device(e, (const Cplx *)device_values, logslots, level, scale, batch, pt);
    });
}

extern "C" int lr_ckks_decode_device(lr_ckks_encoder *e, const lr_poly *pt, int slots, int level, double scale, int batch, void *device_values) {
    return guarded([&]() -> int {
    int logslots = 0;
    LR_TRY(ckks_encoder_check(e, pt, slots, level, scale, batch, &logslots));
    if (!device_values) return fail(LR_ERR_ARG, "null argument");
    LR_HIP(hipSetDevice(e->device));
    return ckks_decode_on_device(e, pt, logslots, level, scale, batch, (Cplx *)device_values);
    });
}
