// The CKKS encoder's host side under AddressSanitizer + UBSan (tests/test_host_ckks_encoder_sanitizers.py): the REAL host code --
// lr_ckks_encoder.cpp with every other host unit of the library -- compiled with g++ against the host-only HIP stand-in and the launch
// stand-ins of tests/cpp/hipstub/, which touch the first and the last word of everything a kernel would read or write.  Both routes (by
// slot count and by lr_options::ckks_encoder_tiled), batches 1 and max_batch (256 at N = 2^4: the one-kernel form of fused Encode), slot
// counts 1, 8 and N / 2, the lowest and the highest level, a caller's root table and the library's, host-value and device-pointer entry
// points, wide plaintext polys, the table builders and every refusal.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "driver_check.hpp"

namespace lr {
extern std::atomic<unsigned long long> g_stub_launches, g_ckks_stub_launches, g_ckks_stub_fused, g_ckks_stub_stages;
}

static const int NQ = 3;

static unsigned long long launches() { return lr::g_stub_launches.load() + lr::g_ckks_stub_launches.load(); }

static int log2_of(uint64_t x) {
    int l = 0;
    while (((uint64_t)1 << l) < x) ++l;
    return l;
}

// the streaming stages of one transform on the tiled route: the tile is a quarter of the slots, at most 2^11
static int tiled_stages(int logslots) {
    const int tile = logslots < 2 ? 0 : (logslots - 2 < 11 ? logslots - 2 : 11);
    return logslots - tile;
}

// one encoder through every call shape; returns the number of accepted calls
static int exercise(lr_context *q, uint64_t N, const lr_options *opt, bool own_roots, bool tiled_option) {
    const int MAXB = N == 16 ? 256 : 5;                                 // 256: the batch from which fused Encode is one kernel
    const uint64_t m = 2 * N;
    std::vector<double> roots(2 * (m + 1));
    for (uint64_t i = 0; i <= m; ++i) {
        roots[2 * i] = std::cos(2 * 3.141592653589793 * (double)(i % m) / (double)m);
        roots[2 * i + 1] = std::sin(2 * 3.141592653589793 * (double)(i % m) / (double)m);
    }
    lr_ckks_encoder *enc = nullptr;
    const double *rp = own_roots ? roots.data() : nullptr;
    OK(opt ? lr_ckks_encoder_create_ex(q, MAXB, rp, opt, &enc) : lr_ckks_encoder_create(q, MAXB, rp, &enc));
    if (!enc) return 0;
    int calls = 0;
    std::vector<uint64_t> rot(m / 2, 99);
    std::vector<double> back(2 * (m + 1), -5.0);
    OK(lr_ckks_encoder_tables(enc, rot.data(), back.data()));
    uint64_t five = 1;
    for (uint64_t i = 0; i < m / 2; ++i) {
        CHECK(rot[i] == (i < m / 4 ? five : 0));
        five = (five * 5) & (m - 1);
    }
    CHECK(back[0] == 1.0 && back[1] == 0.0 && back[2 * m] == 1.0 && back[2 * m + 1] == 0.0);
    if (own_roots) CHECK(std::memcmp(back.data(), roots.data(), back.size() * sizeof(double)) == 0);
    for (int batch : {1, MAXB})
        for (uint64_t slots : {(uint64_t)1, (uint64_t)8, N / 2}) {
            const int logslots = log2_of(slots), level = (batch + logslots) % 2 ? NQ - 1 : 0;
            const bool expect_fused = !tiled_option && logslots <= 13;
            int fused = -1;
            OK(lr_ckks_encoder_route(enc, (int)slots, &fused));
            CHECK(fused == (expect_fused ? 1 : 0));
            const bool wide = batch == 1;                                       // a poly with more limbs than level + 1: another stride
            lr_poly *pt = poly(q, wide ? NQ : level + 1, batch);
            std::vector<double> v((size_t)batch * slots * 2, 0.25), out((size_t)batch * slots * 2);     // exactly [batch][slots] complex128
            const unsigned long long fused_before = lr::g_ckks_stub_fused.load(), stages_before = lr::g_ckks_stub_stages.load(), before = launches();
            OK(lr_ckks_encode(enc, v.data(), (int)slots, level, 1073741824.0, batch, pt));
            OK(lr_ckks_decode(enc, pt, (int)slots, level, 1073741824.0, batch, out.data()));
            void *dv = nullptr, *dout = nullptr;                                // the device-pointer forms: "device" buffers of the exact sizes
            CHECK(hipMalloc(&dv, (size_t)batch * slots * 16) == hipSuccess);
            CHECK(hipMalloc(&dout, (size_t)batch * slots * 16) == hipSuccess);
            OK(lr_ckks_encode_device(enc, dv, (int)slots, level, 1073741824.0, batch, pt));
            OK(lr_ckks_decode_device(enc, pt, (int)slots, level, 1073741824.0, batch, dout));
            OK(lr_context_sync(q));
            calls += 4;
            // fused: encode kernel (from batch 256 on; below it an LDS kernel and the scale-up) + NTT, InvNTT + CRT + one LDS kernel; tiled: the streaming stages, a tile kernel and the scale-up or the CRT
            // (a transform of contextQ may be several launches)
            if (expect_fused) CHECK(launches() - before >= 2 * 2 + 2 * 3);
            else CHECK(launches() - before >= 2 * (tiled_stages(logslots) + 3) + 2 * (tiled_stages(logslots) + 3));
            CHECK(lr::g_ckks_stub_fused.load() - fused_before == (expect_fused && batch >= 256 ? 2ull : 0ull));
            CHECK(lr::g_ckks_stub_stages.load() - stages_before == (expect_fused ? 0ull : 4ull * tiled_stages(logslots)));
            (void)hipFree(dv);
            (void)hipFree(dout);
            lr_poly_free(pt);
        }
    OK(lr_ckks_encoder_destroy(enc));
    return calls;
}

static int refusals(lr_context *q, lr_context *other, uint64_t N) {
    int count = 0;
    lr_ckks_encoder *enc = nullptr, *none = nullptr;
    const unsigned long long before = launches();
    const double s = 1073741824.0;
    // creation
    CHECK(lr_ckks_encoder_create(q, 0, nullptr, &none) == LR_ERR_ARG && none == nullptr);
    CHECK(lr_ckks_encoder_create(q, 65536, nullptr, &none) == LR_ERR_ARG);
    CHECK(lr_ckks_encoder_create(nullptr, 1, nullptr, &none) == LR_ERR_ARG);
    CHECK(lr_ckks_encoder_create(q, 1, nullptr, nullptr) == LR_ERR_ARG);
    lr_options bad;
    OK(lr_options_init(&bad));
    bad.version = 99;
    CHECK(lr_ckks_encoder_create_ex(q, 1, nullptr, &bad, &none) == LR_ERR_ARG);
    count += 5;
    OK(lr_ckks_encoder_create(q, 2, nullptr, &enc));
    std::vector<double> v((size_t)3 * N * 2 + 4);
    std::vector<uint64_t> rot(N);
    lr_poly *pt = poly(q, NQ, 2), *one = poly(q, NQ, 1), *big = poly(q, NQ, 3), *narrow = poly(q, NQ - 1, 2), *foreign = poly(other, NQ, 2);
    int fused = 0;
    for (int bad_slots : {0, -8, 3, 12, (int)N}) {                                               // not a power of two in 1 .. N / 2
        CHECK(lr_ckks_encode(enc, v.data(), bad_slots, 0, s, 2, pt) == LR_ERR_ARG);
        CHECK(lr_ckks_decode(enc, pt, bad_slots, 0, s, 2, v.data()) == LR_ERR_ARG);
        CHECK(lr_ckks_encoder_route(enc, bad_slots, &fused) == LR_ERR_ARG);
        count += 3;
    }
    for (double bad_scale : {0.0, -1.0, (double)INFINITY, (double)NAN}) {
        CHECK(lr_ckks_encode(enc, v.data(), 4, 0, bad_scale, 2, pt) == LR_ERR_ARG);
        CHECK(lr_ckks_decode_device(enc, pt, 4, 0, bad_scale, 2, v.data()) == LR_ERR_ARG);
        count += 2;
    }
    CHECK(lr_ckks_encode(enc, v.data(), 4, 0, s, 2, one) == LR_ERR_SHAPE);                      // batch != the poly's
    CHECK(lr_ckks_decode(enc, one, 4, 0, s, 2, v.data()) == LR_ERR_SHAPE);
    CHECK(lr_ckks_encode(enc, v.data(), 4, 0, s, 0, pt) == LR_ERR_SHAPE);
    CHECK(lr_ckks_encode(enc, v.data(), 4, 0, s, 3, big) == LR_ERR_SHAPE);                      // batch > max_batch
    CHECK(lr_ckks_decode(enc, big, 4, 0, s, 3, v.data()) == LR_ERR_SHAPE);
    CHECK(lr_ckks_encode(enc, v.data(), 4, NQ - 1, s, 2, narrow) == LR_ERR_SHAPE);              // fewer than level + 1 limbs
    CHECK(lr_ckks_decode_device(enc, narrow, 4, NQ - 1, s, 2, v.data()) == LR_ERR_SHAPE);
    CHECK(lr_ckks_encode(enc, v.data(), 4, NQ, s, 2, pt) == LR_ERR_SHAPE);                      // no such level
    CHECK(lr_ckks_decode(enc, pt, 4, -1, s, 2, v.data()) == LR_ERR_SHAPE);
    CHECK(lr_ckks_encode_device(enc, v.data(), 4, 0, s, 2, foreign) == LR_ERR_ARG);             // a poly of another context
    CHECK(lr_ckks_decode(enc, foreign, 4, 0, s, 2, v.data()) == LR_ERR_ARG);
    CHECK(lr_ckks_encode(nullptr, v.data(), 4, 0, s, 2, pt) == LR_ERR_ARG);                     // null pointers
    CHECK(lr_ckks_encode(enc, nullptr, 4, 0, s, 2, pt) == LR_ERR_ARG);
    CHECK(lr_ckks_encode(enc, v.data(), 4, 0, s, 2, nullptr) == LR_ERR_ARG);
    CHECK(lr_ckks_decode(enc, nullptr, 4, 0, s, 2, v.data()) == LR_ERR_ARG);
    CHECK(lr_ckks_decode(enc, pt, 4, 0, s, 2, nullptr) == LR_ERR_ARG);
    CHECK(lr_ckks_encode_device(enc, nullptr, 4, 0, s, 2, pt) == LR_ERR_ARG);
    CHECK(lr_ckks_decode_device(enc, pt, 4, 0, s, 2, nullptr) == LR_ERR_ARG);
    CHECK(lr_ckks_encoder_tables(enc, nullptr, v.data()) == LR_ERR_ARG);
    CHECK(lr_ckks_encoder_tables(nullptr, rot.data(), v.data()) == LR_ERR_ARG);
    CHECK(lr_ckks_encoder_route(enc, 4, nullptr) == LR_ERR_ARG);
    CHECK(lr_ckks_encoder_route(nullptr, 4, &fused) == LR_ERR_ARG);
    count += 22;
    CHECK(launches() == before);                                                                  // no refusal launched anything
    OK(lr_ckks_encode(enc, v.data(), 4, 0, s, 2, pt));                                            // the handle stays usable
    for (lr_poly *p : {pt, one, big, narrow, foreign}) lr_poly_free(p);
    OK(lr_ckks_encoder_destroy(enc));
    OK(lr_ckks_encoder_destroy(nullptr));
    return count;
}

int main() {
    int calls = 0, refused = 0;
    lr_options tiled;
    OK(lr_options_init(&tiled));
    tiled.ckks_encoder_tiled = 1;
    for (uint64_t N : {(uint64_t)1 << 4, (uint64_t)1 << 11, (uint64_t)1 << 15}) {       // N / 2 = 2^14 slots: the tiled route by the slot count
        lr_context *q = nullptr;
        OK(lr_context_create(N, Qm, NQ, 0, &q));
        calls += exercise(q, N, nullptr, true, false);
        calls += exercise(q, N, &tiled, false, true);
        OK(lr_context_destroy(q));
    }
    {
        const uint64_t N = 1 << 4;
        lr_context *q = nullptr, *other = nullptr;
        OK(lr_context_create(N, Qm, NQ, 0, &q));
        OK(lr_context_create(N, Qm, NQ, 0, &other));
        refused += refusals(q, other, N);
        OK(lr_context_destroy(other));
        OK(lr_context_destroy(q));
    }
    return driver_end(ALLOCATIONS | EVENTS, refused, "ckks_encoder: calls %d, refusals %d", calls, refused);
}
