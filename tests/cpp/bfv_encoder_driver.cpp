// The BFV encoder's host side under AddressSanitizer + UBSan (tests/test_host_bfv_encoder_sanitizers.py): the REAL host code --
// lr_bfv_encoder.cpp with every other host unit of the library -- compiled with g++ against the host-only HIP stand-in and the launch
// stand-ins of tests/cpp/hipstub/, which touch the first and the last word of everything a kernel would read or write.  Both routes (by
// shape and by lr_options::bfv_encoder_unfused), batches 1, 3 and max_batch, n_values 0, 1 and N, host-value and device-pointer entry
// points, wide and strided plaintext polys, and every refusal.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "driver_check.hpp"

namespace lr {
extern std::atomic<unsigned long long> g_stub_launches, g_encoder_stub_launches, g_encoder_stub_fused;
}

static const int NQ = 3, MAXB = 5;
static const uint64_t T40 = 1099515691009ull;     // a plaintext modulus of 2^31 and more: the composed route whatever N

static unsigned long long launches() { return lr::g_stub_launches.load() + lr::g_encoder_stub_launches.load(); }

// one encoder through every call shape; returns the number of accepted calls
static int exercise(lr_context *q, uint64_t N, uint64_t t, const lr_options *opt, bool expect_fused) {
    lr_bfv_encoder *enc = nullptr;
    OK(opt ? lr_bfv_encoder_create_ex(q, t, MAXB, opt, &enc) : lr_bfv_encoder_create(q, t, MAXB, &enc));
    if (!enc) return 0;
    int fused = -1, calls = 0;
    OK(lr_bfv_encoder_route(enc, &fused));
    CHECK(fused == (expect_fused ? 1 : 0));
    std::vector<uint64_t> index(N), delta(NQ);
    OK(lr_bfv_encoder_tables(enc, index.data(), delta.data()));
    std::vector<bool> seen(N, false);
    for (uint64_t i : index) {
        CHECK(i < N && !seen[i]);
        if (i < N) seen[i] = true;
    }
    for (int batch : {1, 3, MAXB})
        for (size_t n : {(size_t)0, (size_t)1, (size_t)N}) {
            const bool wide = (batch + n) % 2 == 1;                       // a poly with one limb more than |Q|: another stride
            lr_poly *pt = poly(q, wide ? NQ + 1 : NQ, batch);
            std::vector<uint64_t> u(batch * n + 1, 7);                    // exactly [batch][n_values] (+1: data() of an empty vector)
            std::vector<int64_t> s(batch * n + 1, -7);
            std::vector<uint64_t> du((size_t)batch * N);
            std::vector<int64_t> ds((size_t)batch * N);
            const unsigned long long fused_before = lr::g_encoder_stub_fused.load(), before = launches();
            OK(lr_bfv_encode_uint(enc, n ? u.data() : nullptr, n, batch, pt));
            OK(lr_bfv_encode_int(enc, s.data(), n, batch, pt));
            OK(lr_bfv_decode_uint(enc, pt, batch, du.data()));
            OK(lr_bfv_decode_int(enc, pt, batch, ds.data()));
            // the device-pointer forms: "device" buffers of the exact sizes
            void *dv = nullptr, *dout = nullptr;
            CHECK(hipMalloc(&dv, (size_t)batch * n * 8) == hipSuccess);
            CHECK(hipMalloc(&dout, (size_t)batch * N * 8) == hipSuccess);
            OK(lr_bfv_encode_device(enc, dv, n, batch, 0, pt));
            OK(lr_bfv_encode_device(enc, dv, n, batch, 1, pt));
            OK(lr_bfv_decode_device(enc, pt, batch, 0, dout));
            OK(lr_bfv_decode_device(enc, pt, batch, 1, dout));
            OK(lr_context_sync(q));
            calls += 8;
            // fused: 1 launch per encode, scale + 1 per decode; composed: scatter, InvNTT, lift / scale, NTT, gather
            // (a transform of the composed route may be several launches: sub-blocks and a top stage)
            if (expect_fused) CHECK(launches() - before == 4 * 1 + 4 * 2);
            else CHECK(launches() - before >= 4 * 3 + 4 * 3);
            CHECK(lr::g_encoder_stub_fused.load() - fused_before == (expect_fused ? 8ull : 0ull));
            (void)hipFree(dv);
            (void)hipFree(dout);
            lr_poly_free(pt);
        }
    OK(lr_bfv_encoder_destroy(enc));
    return calls;
}

static int refusals(lr_context *q, lr_context *other, uint64_t N) {
    int count = 0;
    lr_bfv_encoder *enc = nullptr, *none = nullptr;
    const unsigned long long before = launches();
    // creation
    CHECK(lr_bfv_encoder_create(q, 17, 1, &none) == LR_ERR_NOT_NTT_FRIENDLY && none == nullptr);
    {
        const std::string msg = lr_last_error_string();
        lr_context *c17 = nullptr;
        const uint64_t t17 = 17;
        CHECK(lr_context_create(N, &t17, 1, 0, &c17) == LR_ERR_NOT_NTT_FRIENDLY && msg == lr_last_error_string());
    }
    CHECK(lr_bfv_encoder_create(q, 0, 1, &none) == LR_ERR_ARG);
    CHECK(lr_bfv_encoder_create(q, 65537, 0, &none) == LR_ERR_ARG);
    CHECK(lr_bfv_encoder_create(nullptr, 65537, 1, &none) == LR_ERR_ARG);
    CHECK(lr_bfv_encoder_create(q, 65537, 1, nullptr) == LR_ERR_ARG);
    lr_options bad;
    OK(lr_options_init(&bad));
    bad.version = 99;
    CHECK(lr_bfv_encoder_create_ex(q, 65537, 1, &bad, &none) == LR_ERR_ARG);
    count += 6;
    OK(lr_bfv_encoder_create(q, 65537, 2, &enc));
    std::vector<uint64_t> v((size_t)3 * (N + 1)), index(N), delta(NQ);
    lr_poly *pt = poly(q, NQ, 2), *one = poly(q, NQ, 1), *big = poly(q, NQ, 3), *narrow = poly(q, NQ - 1, 2), *foreign = poly(other, NQ, 2);
    const int64_t *sv = (const int64_t *)v.data();
    CHECK(lr_bfv_encode_uint(enc, v.data(), N + 1, 2, pt) == LR_ERR_SHAPE);           // n_values > N
    CHECK(lr_bfv_encode_int(enc, sv, N + 1, 2, pt) == LR_ERR_SHAPE);
    CHECK(lr_bfv_encode_device(enc, v.data(), N + 1, 2, 0, pt) == LR_ERR_SHAPE);
    CHECK(lr_bfv_encode_uint(enc, v.data(), 4, 2, one) == LR_ERR_SHAPE);              // batch != the poly's
    CHECK(lr_bfv_decode_uint(enc, one, 2, v.data()) == LR_ERR_SHAPE);
    CHECK(lr_bfv_encode_uint(enc, v.data(), 4, 0, pt) == LR_ERR_SHAPE);
    CHECK(lr_bfv_encode_uint(enc, v.data(), 4, 3, big) == LR_ERR_SHAPE);              // batch > max_batch
    CHECK(lr_bfv_decode_int(enc, big, 3, (int64_t *)v.data()) == LR_ERR_SHAPE);
    CHECK(lr_bfv_encode_uint(enc, v.data(), 4, 2, narrow) == LR_ERR_SHAPE);           // fewer than |Q| limbs
    CHECK(lr_bfv_decode_device(enc, narrow, 2, 0, v.data()) == LR_ERR_SHAPE);
    CHECK(lr_bfv_encode_int(enc, sv, 4, 2, foreign) == LR_ERR_ARG);                   // a poly of another context
    CHECK(lr_bfv_decode_uint(enc, foreign, 2, v.data()) == LR_ERR_ARG);
    CHECK(lr_bfv_encode_uint(nullptr, v.data(), 4, 2, pt) == LR_ERR_ARG);             // null pointers
    CHECK(lr_bfv_encode_uint(enc, nullptr, 4, 2, pt) == LR_ERR_ARG);
    CHECK(lr_bfv_encode_int(enc, sv, 4, 2, nullptr) == LR_ERR_ARG);
    CHECK(lr_bfv_decode_uint(enc, nullptr, 2, v.data()) == LR_ERR_ARG);
    CHECK(lr_bfv_decode_int(enc, pt, 2, nullptr) == LR_ERR_ARG);
    CHECK(lr_bfv_encode_device(enc, nullptr, 4, 2, 1, pt) == LR_ERR_ARG);
    CHECK(lr_bfv_decode_device(enc, pt, 2, 1, nullptr) == LR_ERR_ARG);
    CHECK(lr_bfv_encoder_tables(enc, nullptr, delta.data()) == LR_ERR_ARG);
    CHECK(lr_bfv_encoder_tables(nullptr, index.data(), delta.data()) == LR_ERR_ARG);
    CHECK(lr_bfv_encoder_route(enc, nullptr) == LR_ERR_ARG);
    count += 22;
    CHECK(launches() == before);                                                        // no refusal launched anything
    OK(lr_bfv_encode_uint(enc, v.data(), 4, 2, pt));                                    // the handle stays usable
    for (lr_poly *p : {pt, one, big, narrow, foreign}) lr_poly_free(p);
    OK(lr_bfv_encoder_destroy(enc));
    OK(lr_bfv_encoder_destroy(nullptr));
    return count;
}

int main() {
    int calls = 0, refused = 0;
    lr_options unfused;
    OK(lr_options_init(&unfused));
    unfused.bfv_encoder_unfused = 1;
    for (uint64_t N : {(uint64_t)1 << 11, (uint64_t)1 << 15}) {
        lr_context *q = nullptr;
        OK(lr_context_create(N, Qm, NQ, 0, &q));
        calls += exercise(q, N, 65537, nullptr, true);           // the fused route by shape
        calls += exercise(q, N, 65537, &unfused, false);         // the composed route by the option field
        calls += exercise(q, N, T40, nullptr, false);            // ... by the modulus
        OK(lr_context_destroy(q));
    }
    {
        const uint64_t N = 1 << 4;                               // below the fused kernels' lower bound
        lr_context *q = nullptr, *other = nullptr;
        OK(lr_context_create(N, Qm, NQ, 0, &q));
        OK(lr_context_create(N, Qm, NQ, 0, &other));
        calls += exercise(q, N, 65537, nullptr, false);
        refused += refusals(q, other, N);
        OK(lr_context_destroy(other));
        OK(lr_context_destroy(q));
    }
    return driver_end(ALLOCATIONS | EVENTS, refused, "bfv_encoder: calls %d, refusals %d", calls, refused);
}
