// lr_bfv_encoder.cpp -- C ABI: lr_bfv_encoder, bfv.Encoder (bfv/encoder.go:28-182) for a batch of plaintexts on the device.
// The host sanitizer build (tests/host_stub_build.py) compiles this unit with every other; the launchers of lr_bfv_encode.hip have their
// stand-in in tests/cpp/hipstub/stub_bfv_encode.cpp.
#include "lr_host.hpp"

// what bfv.NewEncoder builds (bfv/encoder.go:28-68), plus the staging of the host-value entry points
struct lr_bfv_encoder {
    int device = 0;
    lr_context *cQ = nullptr;
    lr_context *cT = nullptr;                 // contextT = (N, [t]), owned: its psi tables are the reference's
    lr_simple_scaler *scaler = nullptr;       // NewSimpleScaler(t, contextQ), owned
    u64 t = 0;
    int max_batch = 0;
    bool fused = false;                       // the route, decided once at creation (encoder_fused_shape, Options::bfv_encoder_unfused)
    std::vector<u64> index_matrix, delta_mont;
    u32 *d_index = nullptr;
    u64 *d_delta = nullptr;
    Tw32 *d_tw_inv = nullptr, *d_tw_fwd = nullptr;   // fused route only
    Tw32 n_inv{0, 0};
    u64 *d_row = nullptr;                     // polypool: one limb over t for max_batch plaintexts, [max_batch][N]
    u64 *d_values = nullptr;                  // the host-value entry points' slots on the device, [max_batch][N]
    u64 *h_values = nullptr;                  // the same, pinned
    hipEvent_t staged = nullptr;              // the last copy out of h_values: the next call waits for it before it refills the buffer
    ~lr_bfv_encoder() {
        for (void *p : {(void *)d_index, (void *)d_delta, (void *)d_tw_inv, (void *)d_tw_fwd, (void *)d_row, (void *)d_values})
            if (p) (void)hipFree(p);
        if (h_values) (void)hipHostFree(h_values);
        if (staged) (void)hipEventDestroy(staged);
        if (scaler) lr_simple_scaler_destroy(scaler);
        if (cT) lr_context_destroy(cT);
    }
};

namespace lr_host {
namespace {

// The route decision: the fused kernels hold the transform in 4 N bytes of one CU's LDS (N <= 2^15), give each of their 1024 threads at
// least one butterfly per stage (N >= 2^11) and keep sums of two canonical values in 32 bits (t < 2^31); DESIGN.md 3.5.
bool encoder_fused_shape(const HostContext &hT) { return hT.logN >= 11 && hT.logN <= 15 && hT.q[0] < (1ull << 31); }

// a power of psi out of the [t] context's Montgomery-form table, in the fused kernels' 32-bit Shoup form
Tw32 tw32_of(u64 mont, const HostContext &hT) {
    const u64 t = hT.q[0], w = inv_mform(mont, t, hT.mred[0]);
    return Tw32{(u32)w, (u32)((w << 32) / t)};
}

EncoderTables encoder_tables(const lr_bfv_encoder *e) {
    EncoderTables tab;
    tab.index = e->d_index;
    tab.t = e->t;
    tab.t_bred_hi = e->cT->h.bred[0].hi;
    tab.n = (int)e->cT->h.N;
    tab.logn = (int)e->cT->h.logN;
    return tab;
}

// null handles, the batch against the poly and max_batch, the poly against contextQ
int encoder_check(const lr_bfv_encoder *e, const lr_poly *pt, int batch) {
    if (!e || !pt) return fail(LR_ERR_ARG, "null argument");
    if (pt->ctx != e->cQ) return fail(LR_ERR_ARG, "BFV encoder: the plaintext poly belongs to another context");
    if (pt->N != e->cQ->h.N || pt->limbs < e->cQ->h.L()) return fail(LR_ERR_SHAPE, "BFV encoder: the plaintext poly must hold |Q| limbs");
    if (batch < 1 || batch != pt->batch) return fail(LR_ERR_SHAPE, "BFV encoder: batch differs from the plaintext poly's");
    if (batch > e->max_batch) return fail(LR_ERR_SHAPE, "batch exceeds the encoder's max_batch");
    return LR_OK;
}

// contextT runs on contextQ's stream of the moment.  Its work only ever goes out through this handle, between launches on contextQ's
// stream, and lr_context_set_stream has ordered that stream behind the one contextQ had before: no event of its own is needed (nor
// possible: the earlier stream may be the caller's and gone).
hipStream_t encoder_stream(lr_bfv_encoder *e) {
    e->cT->stream = e->cQ->stream;
    return e->cQ->stream;
}

// EncodeUint / EncodeInt (bfv/encoder.go:70-137) of slots already on the device
int encode_on_device(lr_bfv_encoder *e, const void *d_values, size_t n_values, int batch, int is_signed, lr_poly *pt) {
    const HostContext &hQ = e->cQ->h;
    hipStream_t s = encoder_stream(e);
    const EncoderTables tab = encoder_tables(e);
    if (e->fused) {
        EncodeLaunch L;
        L.tab = tab;
        L.values = d_values;
        L.n_values = (long long)n_values;
        L.is_signed = is_signed;
        L.tw_inv = e->d_tw_inv;
        L.n_inv = e->n_inv;
        L.out = pt->d;
        L.out_stride = pt->stride();
        L.limbs = hQ.L();
        L.lp = e->cQ->d_lp;
        L.delta_mont = e->d_delta;
        LR_HIP(launch_bfv_encode_fused(L, batch, s));
        return LR_OK;
    }
    LR_HIP(launch_bfv_slot_scatter(tab, d_values, (long long)n_values, is_signed, e->d_row, batch, s));
    const Rows row{e->d_row, (long long)hQ.N, 0, 1};
    LR_TRY(run_ntt(e->cT, true, row, row, 0, 1, 1, batch));
    LR_HIP(launch_bfv_lift(e->d_row, (int)hQ.N, pt->d, pt->stride(), hQ.L(), e->cQ->d_lp, e->d_delta, batch, s));
    return LR_OK;
}

// DecodeUint / DecodeInt (bfv/encoder.go:139-182) into slots on the device
int decode_on_device(lr_bfv_encoder *e, const lr_poly *pt, int batch, int is_signed, void *d_values) {
    const HostContext &hQ = e->cQ->h;
    hipStream_t s = encoder_stream(e);
    const EncoderTables tab = encoder_tables(e);
    ScaleLaunch S;                                        // simplescaler.Scale(plaintext.value, polypool), :142
    S.in = pt->d;
    S.out = e->d_row;
    S.in_stride = pt->stride();
    S.out_stride = (long long)hQ.N;
    S.wi = e->scaler->d_wi;
    S.ti = e->scaler->d_ti;
    S.t = e->scaler->h.t;
    S.add_param = e->scaler->h.add_param;
    S.mul_param = e->scaler->h.mul_param;
    S.pow2 = e->scaler->h.pow2 ? 1 : 0;
    S.limbs_in = hQ.L();
    S.limbs_out = 1;
    S.n = (int)hQ.N;
    LR_HIP(launch_simple_scale(S, batch, s));
    if (e->fused) {
        DecodeLaunch L;
        L.tab = tab;
        L.in = e->d_row;
        L.tw_fwd = e->d_tw_fwd;
        L.values = d_values;
        L.is_signed = is_signed;
        LR_HIP(launch_bfv_decode_fused(L, batch, s));
        return LR_OK;
    }
    const Rows row{e->d_row, (long long)hQ.N, 0, 1};
    LR_TRY(run_ntt(e->cT, false, row, row, 0, 1, 1, batch));
    LR_HIP(launch_bfv_slot_gather(tab, e->d_row, d_values, is_signed, batch, s));
    return LR_OK;
}

// the caller's slots through the pinned buffer to the device; the caller's array is free on return
int stage_values_in(lr_bfv_encoder *e, const void *values, size_t words) {
    if (words == 0) return LR_OK;
    LR_HIP(hipEventSynchronize(e->staged));               // the copy of the call before has left the pinned buffer
    std::memcpy(e->h_values, values, words * sizeof(u64));
    LR_HIP(hipMemcpyAsync(e->d_values, e->h_values, words * sizeof(u64), hipMemcpyHostToDevice, e->cQ->stream));
    LR_HIP(hipEventRecord(e->staged, e->cQ->stream));
    return LR_OK;
}

int encode_host(lr_bfv_encoder *e, const void *values, size_t n_values, int batch, int is_signed, lr_poly *pt) {
    LR_TRY(encoder_check(e, pt, batch));
    if (n_values > e->cQ->h.N) return fail(LR_ERR_SHAPE, "BFV encoder: more values than slots (bfv/encoder.go:73)");
    if (!values && n_values) return fail(LR_ERR_ARG, "null argument");
    LR_HIP(hipSetDevice(e->device));
    LR_TRY(stage_values_in(e, values, (size_t)batch * n_values));
    return encode_on_device(e, e->d_values, n_values, batch, is_signed, pt);
}

int decode_host(lr_bfv_encoder *e, const lr_poly *pt, int batch, int is_signed, void *values) {
    LR_TRY(encoder_check(e, pt, batch));
    if (!values) return fail(LR_ERR_ARG, "null argument");
    LR_HIP(hipSetDevice(e->device));
    LR_TRY(decode_on_device(e, pt, batch, is_signed, e->d_values));
    const size_t bytes = (size_t)batch * e->cQ->h.N * sizeof(u64);
    LR_HIP(hipEventSynchronize(e->staged));
    LR_HIP(hipMemcpyAsync(e->h_values, e->d_values, bytes, hipMemcpyDeviceToHost, e->cQ->stream));
    LR_HIP(hipStreamSynchronize(e->cQ->stream));
    std::memcpy(values, e->h_values, bytes);
    return LR_OK;
}

}  // namespace
}  // namespace lr_host

extern "C" int lr_bfv_encoder_create(lr_context *cQ, uint64_t t, int max_batch, lr_bfv_encoder **out) {
    return lr_bfv_encoder_create_ex(cQ, t, max_batch, nullptr, out);
}

extern "C" int lr_bfv_encoder_create_ex(lr_context *cQ, uint64_t t, int max_batch, const lr_options *options, lr_bfv_encoder **out) {
    return guarded([&]() -> int {
    if (!cQ || !out) return fail(LR_ERR_ARG, "null argument");
    *out = nullptr;
    Options parsed = cQ->opt;
    if (options) LR_TRY(options_from_public(options, &parsed));
    else parsed.apply_env();
    if (max_batch < 1 || max_batch > 65535) return fail(LR_ERR_ARG, "max_batch must be in 1 .. 65535");
    if (t == 0) return fail(LR_ERR_ARG, "t must be non-zero (BRedParams divides by it, ring/modular_reduction.go:97)");
    std::unique_ptr<lr_bfv_encoder> e(new lr_bfv_encoder());
    e->cQ = cQ;
    e->device = cQ->device;
    e->t = t;
    e->max_batch = max_batch;
    // contextT: a t that does not allow an NTT at N is lr_context_create's refusal, code and message
    lr_options topt;
    options_to_public(parsed, &topt);
    LR_TRY(lr_context_create_ex(cQ->h.N, &t, 1, cQ->device, &topt, &e->cT));
    LR_TRY(lr_simple_scaler_create(cQ, t, &e->scaler));
    const HostContext &hT = e->cT->h;
    const size_t N = (size_t)hT.N;
    e->fused = encoder_fused_shape(hT) && !parsed.bfv_encoder_unfused;
    e->index_matrix = build_index_matrix(hT.N, hT.logN);
    e->delta_mont = build_lift_params(cQ->h, t);
    LR_HIP(hipSetDevice(cQ->device));
    std::vector<u32> index32(e->index_matrix.begin(), e->index_matrix.end());
    LR_TRY(to_device(&e->d_index, index32.data(), N));
    LR_TRY(to_device(&e->d_delta, e->delta_mont.data(), e->delta_mont.size()));
    if (e->fused) {
        std::vector<Tw32> inv(N), fwd(N);
        for (size_t k = 0; k < N; ++k) {
            inv[k] = tw32_of(hT.ntt_psi_inv[k], hT);
            fwd[k] = tw32_of(hT.ntt_psi[k], hT);
        }
        e->n_inv = tw32_of(hT.n_inv[0], hT);
        LR_TRY(to_device(&e->d_tw_inv, inv.data(), N));
        LR_TRY(to_device(&e->d_tw_fwd, fwd.data(), N));
    }
    const size_t words = (size_t)max_batch * N;
    LR_HIP(hipMalloc((void **)&e->d_row, words * sizeof(u64)));
    LR_HIP(hipMalloc((void **)&e->d_values, words * sizeof(u64)));
    LR_HIP(hipHostMalloc((void **)&e->h_values, words * sizeof(u64), 0));
    LR_HIP(hipEventCreateWithFlags(&e->staged, hipEventDisableTiming));
    *out = e.release();
    return LR_OK;
    });
}

extern "C" int lr_bfv_encoder_destroy(lr_bfv_encoder *e) {
    return guarded([&]() -> int {
    if (!e) return LR_OK;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();   // the handle's work may be on its context's caller-supplied stream
    delete e;
    return LR_OK;
    });
}

extern "C" int lr_bfv_encoder_tables(const lr_bfv_encoder *e, uint64_t *index_matrix, uint64_t *delta_mont) {
    return guarded([&]() -> int {
    if (!e || !index_matrix || !delta_mont) return fail(LR_ERR_ARG, "null argument");
    std::copy(e->index_matrix.begin(), e->index_matrix.end(), index_matrix);
    std::copy(e->delta_mont.begin(), e->delta_mont.end(), delta_mont);
    return LR_OK;
    });
}

extern "C" int lr_bfv_encoder_route(const lr_bfv_encoder *e, int *fused) {
    return guarded([&]() -> int {
    if (!e || !fused) return fail(LR_ERR_ARG, "null argument");
    *fused = e->fused ? 1 : 0;
    return LR_OK;
    });
}

extern "C" int lr_bfv_encode_uint(lr_bfv_encoder *e, const uint64_t *values, size_t n_values, int batch, lr_poly *pt) {
    return guarded([&]() -> int { return encode_host(e, values, n_values, batch, 0, pt); });
}

extern "C" int lr_bfv_encode_int(lr_bfv_encoder *e, const int64_t *values, size_t n_values, int batch, lr_poly *pt) {
    return guarded([&]() -> int { return encode_host(e, values, n_values, batch, 1, pt); });
}

extern "C" int lr_bfv_decode_uint(lr_bfv_encoder *e, const lr_poly *pt, int batch, uint64_t *values) {
    return guarded([&]() -> int { return decode_host(e, pt, batch, 0, values); });
}

extern "C" int lr_bfv_decode_int(lr_bfv_encoder *e, const lr_poly *pt, int batch, int64_t *values) {
    return guarded([&]() -> int { return decode_host(e, pt, batch, 1, values); });
}

extern "C" int lr_bfv_encode_device(lr_bfv_encoder *e, const void *device_values, size_t n_values, int batch, int is_signed, lr_poly *pt) {
    return guarded([&]() -> int {
    LR_TRY(encoder_check(e, pt, batch));
    if (n_values > e->cQ->h.N) return fail(LR_ERR_SHAPE, "BFV encoder: more values than slots (bfv/encoder.go:73)");
    if (!device_values && n_values) return fail(LR_ERR_ARG, "null argument");
    LR_HIP(hipSetDevice(e->device));
    return encode_on_device(e, device_values, n_values, batch, is_signed ? 1 : 0, pt);
    });
}

extern "C" int lr_bfv_decode_device(lr_bfv_encoder *e, const lr_poly *pt, int batch, int is_signed, void *device_values) {
    return guarded([&]() -> int {
    LR_TRY(encoder_check(e, pt, batch));
    if (!device_values) return fail(LR_ERR_ARG, "null argument");
    LR_HIP(hipSetDevice(e->device));
    return decode_on_device(e, pt, batch, is_signed ? 1 : 0, device_values);
    });
}
