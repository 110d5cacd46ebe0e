// The key generator's host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_keygen_sanitizers.py): the REAL
// host code -- lr_keygen.cpp with every other host unit of the library -- compiled with g++ against the host-only HIP stand-in and the
// launch stand-ins of tests/cpp/hipstub/, which touch the first and the last byte of everything a kernel would read or write.  Every entry
// point in its host and device-pointer form, both shapes (lr_options::no_epilogue), 1, 3 and max_batch keys (5, and 70: more than one pass)
// with the pool and the staging buffer reused across consecutive host-form calls, wide polys, shared and per-key secret keys, |P| = 1 and a
// ragged |P| = 2 whose last digit owns one row; two handles on two threads; the launch counts of both shapes; every refusal.
// Exit code 0 = every check held; a sanitizer report aborts the run.  Nothing here computes: parity is the GPU suite's business.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#define REFUSED REFUSED_MSG      // here a refusal is logged with its message
#include "driver_check.hpp"

namespace lr {
extern std::atomic<unsigned long long> g_stub_launches, g_ckks_expand_launches, g_keygen_skin_launches, g_keygen_finish_launches, g_keygen_pk_launches;
}  // namespace lr

static const int MAXB = 5;

// one key generator through every entry point; returns the number of accepted calls
// max_keys above kKeygenKeysPerLaunch (32): the call runs as several passes over the pool, each with its own offsets into the bytes, the
// secret keys, the Galois elements and the key array
static int exercise(uint64_t N, int nq, int np, const lr_options *opt, int max_keys = MAXB) {
    Rings r(N, Qm, nq, np, opt);
    const int rows = nq + np, beta = (nq + np - 1) / np;
    lr_keygen *kg = nullptr;
    OK(opt ? lr_keygen_create_ex(r.q, r.p, max_keys, opt, &kg) : lr_keygen_create(r.q, r.p, max_keys, &kg));
    if (!kg) return 0;
    int calls = 0;
    for (int round = 0; round < 2; ++round)                                   // the second round reuses the pool and the staging buffer
        for (int n : {1, 3, max_keys}) {
            const bool wide = (n + round) % 2 == 1;                           // polys with one limb more than needed: another stride
            const int kb = round == 0 ? 1 : n;                                // secret keys: one for the call, or one per key
            lr_poly *sk = poly(r.q, rows + (wide ? 1 : 0), n), *sk1 = poly(r.q, rows, 1), *skin = poly(r.q, rows + (wide ? 0 : 1), kb), *skout = poly(r.q, rows, kb);
            lr_poly *pk0 = poly(r.q, rows + (wide ? 1 : 0), n), *pk1 = poly(r.q, rows, n);
            std::vector<lr_poly *> keys;
            for (int k = 0; k < n; ++k) keys.push_back(poly(r.q, rows + ((k + (wide ? 1 : 0)) % 2), 2 * beta));
            // exactly [n][N / 8], [n][N] and [n][beta][N] bytes
            std::vector<uint8_t> bits((size_t)n * N / 8, 0xAA), e1((size_t)n * N, 0x93), e((size_t)n * beta * N, 0x80);
            std::vector<uint64_t> gens;
            for (int k = 0; k < n; ++k) gens.push_back(k % 2 ? 2 * N - 1 : 5);
            void *dbits = nullptr, *de1 = nullptr, *de = nullptr;
            CHECK(hipMalloc(&dbits, bits.size()) == hipSuccess && hipMalloc(&de1, e1.size()) == hipSuccess && hipMalloc(&de, e.size()) == hipSuccess);
            // two host-form calls one behind the other: the second refills the pinned buffer the first one staged through
            OK(lr_keygen_secret_key(kg, bits.data(), bits.data(), n, sk));
            OK(lr_keygen_public_key(kg, kb == 1 ? sk1 : sk, e1.data(), n, pk0, pk1));
            OK(lr_keygen_switching_keys(kg, skin, skout, e.data(), n, keys.data()));
            OK(lr_keygen_relin_keys(kg, sk1, n, e.data(), keys.data()));
            OK(lr_keygen_rotation_keys(kg, sk1, gens.data(), n, e.data(), keys.data()));
            OK(lr_keygen_secret_key_device(kg, dbits, dbits, n, sk));
            OK(lr_keygen_public_key_device(kg, kb == 1 ? sk1 : sk, de1, n, pk0, pk1));
            OK(lr_keygen_switching_keys_device(kg, skin, skout, de, n, keys.data()));
            OK(lr_keygen_relin_keys_device(kg, sk1, n, de, keys.data()));
            OK(lr_keygen_rotation_keys_device(kg, sk1, gens.data(), n, de, keys.data()));
            calls += 10;
            OK(lr_context_sync(r.q));
            for (void *p : {dbits, de1, de}) (void)hipFree(p);
            for (lr_poly *p : {sk, sk1, skin, skout, pk0, pk1}) lr_poly_free(p);
            for (lr_poly *p : keys) lr_poly_free(p);
        }
    OK(lr_keygen_destroy(kg));
    return calls;
}

// at N = 2^4 a transform is one launch per context: the default shape of a switching-key call is expansion, transform, skIn, finish -- ONE
// launch each for all keys -- and the call-by-call shape the reference's Context calls per key and digit
static void sequences() {
    const uint64_t N = 16;
    const int nq = 3, np = 2, beta = 2, n = 3;
    for (int call_by_call : {0, 1}) {
        lr_options opt;
        OK(lr_options_init(&opt));
        opt.no_epilogue = call_by_call;
        Rings r(N, Qm, nq, np, &opt);
        lr_keygen *kg = nullptr;
        OK(lr_keygen_create_ex(r.q, r.p, n, &opt, &kg));
        lr_poly *sk = poly(r.q, nq + np, 1), *pk0 = poly(r.q, nq + np, 1), *pk1 = poly(r.q, nq + np, 1);
        std::vector<lr_poly *> keys;
        for (int k = 0; k < n; ++k) keys.push_back(poly(r.q, nq + np, 2 * beta));
        std::vector<uint8_t> e((size_t)n * beta * N, 0x80);
        const uint64_t gens[3] = {5, 2 * N - 1, 1};
        auto snap = [] {
            return std::vector<unsigned long long>{lr::g_stub_launches.load(), lr::g_ckks_expand_launches.load(), lr::g_keygen_skin_launches.load(),
                                                   lr::g_keygen_finish_launches.load(), lr::g_keygen_pk_launches.load()};
        };
        auto diff = [&](const std::vector<unsigned long long> &a) {
            std::vector<unsigned long long> b = snap();
            for (size_t i = 0; i < b.size(); ++i) b[i] -= a[i];
            return b;
        };
        auto s = snap();
        OK(lr_keygen_rotation_keys(kg, sk, gens, n, e.data(), keys.data()));
        auto d = diff(s);
        if (call_by_call) {
            // the transforms over Q and P; per key PermuteNTT and MulScalarBigint; per digit MForm (Q, P), Add, MulCoeffsMontgomeryAndSub (Q, P)
            CHECK(d[1] == 1 && d[2] == 0 && d[3] == 0 && d[0] == 2 + n * 2 + n * beta * 5);
        } else {
            CHECK(d[1] == 1 && d[2] == 1 && d[3] == 1 && d[0] == 2);
        }
        s = snap();
        OK(lr_keygen_relin_keys(kg, sk, 2, e.data(), keys.data()));
        d = diff(s);
        if (call_by_call) CHECK(d[1] == 1 && d[2] == 0 && d[3] == 0 && d[0] == 2 + 3 + 2 * beta * 5);      // MulScalarBigint, two MulCoeffsMontgomery
        else CHECK(d[1] == 1 && d[2] == 1 && d[3] == 1 && d[0] == 2);
        s = snap();
        OK(lr_keygen_public_key(kg, sk, e.data(), 1, pk0, pk1));
        d = diff(s);
        if (call_by_call) CHECK(d[1] == 1 && d[4] == 0 && d[0] == 2 + 4);                                   // MulCoeffsMontgomeryAndAdd and Neg over Q and P
        else CHECK(d[1] == 1 && d[4] == 1 && d[0] == 2);
        for (lr_poly *p : {sk, pk0, pk1}) lr_poly_free(p);
        for (lr_poly *p : keys) lr_poly_free(p);
        OK(lr_keygen_destroy(kg));
    }
}

static int refusals() {
    const uint64_t N = 16;
    const int nq = 3, np = 1, rows = 4, beta = 3;
    int count = 0;
    Rings r(N, Qm, nq, np, nullptr), other(N, Qm, nq, np, nullptr);
    lr_context *small = nullptr, *big = nullptr, *dev1 = nullptr;
    OK(lr_context_create(4, Qm, nq, 0, &small));
    OK(lr_context_create(2 * N, Qm + nq, np, 0, &big));
    OK(lr_context_create(N, Qm + nq, np, 1, &dev1));
    lr_keygen *kg = nullptr, *none = nullptr, *no_p = nullptr;
    const unsigned long long before = lr::g_stub_launches.load() + lr::g_ckks_expand_launches.load();
    // creation
    REFUSED(lr_keygen_create(nullptr, r.p, 1, &none) == LR_ERR_ARG);
    REFUSED(lr_keygen_create(r.q, r.p, 1, nullptr) == LR_ERR_ARG);
    REFUSED(lr_keygen_create(r.q, r.p, 0, &none) == LR_ERR_ARG && none == nullptr);
    REFUSED(lr_keygen_create(r.q, r.p, 65536, &none) == LR_ERR_ARG);
    REFUSED(lr_keygen_create(small, nullptr, 1, &none) == LR_ERR_ARG);                 // N < 8
    REFUSED(lr_keygen_create(r.q, big, 1, &none) == LR_ERR_ARG);                       // ctxP with another N
    REFUSED(lr_keygen_create(r.q, dev1, 1, &none) == LR_ERR_ARG);                      // ctxP on another device
    lr_options bad;
    OK(lr_options_init(&bad));
    bad.version = 99;
    REFUSED(lr_keygen_create_ex(r.q, r.p, 1, &bad, &none) == LR_ERR_ARG);
    count += 8;
    OK(lr_keygen_create(r.q, r.p, 2, &kg));
    OK(lr_keygen_create(r.q, nullptr, 2, &no_p));
    lr_poly *sk = poly(r.q, rows, 1), *sk2 = poly(r.q, rows, 2), *sk3 = poly(r.q, rows, 3), *pk0 = poly(r.q, rows, 2), *pk1 = poly(r.q, rows, 2);
    lr_poly *foreign = poly(other.q, rows, 2), *foreign1 = poly(other.q, rows, 1), *narrow = poly(r.q, rows - 1, 2), *narrow1 = poly(r.q, rows - 1, 1);
    lr_poly *k0 = poly(r.q, rows, 2 * beta), *k1 = poly(r.q, rows, 2 * beta), *k2 = poly(r.q, rows, 2 * beta), *kf = poly(other.q, rows, 2 * beta);
    lr_poly *kn = poly(r.q, rows - 1, 2 * beta), *kb = poly(r.q, rows, 2 * beta - 1), *skq = poly(r.q, nq, 2);
    lr_poly *inside = nullptr;
    {
        uint64_t *d = nullptr;
        OK(lr_poly_info(k0, nullptr, nullptr, nullptr, (void **)&d));
        OK(lr_poly_wrap(r.q, d + (size_t)rows * N, rows, 1, &inside));               // member 1 of k0
    }
    lr_poly *keys[2] = {k0, k1}, *same[2] = {k0, k0}, *with_null[2] = {k0, nullptr}, *with_foreign[2] = {k0, kf}, *with_narrow[2] = {k0, kn},
            *with_batch[2] = {k0, kb}, *three[3] = {k0, k1, k2};
    std::vector<uint8_t> b((size_t)3 * beta * N, 0);
    const uint8_t *u = b.data();
    const uint64_t g[3] = {5, 25, 125}, even[2] = {5, 6}, zero[2] = {0, 5};
    // a handle without P
    REFUSED(lr_keygen_switching_keys(no_p, sk, sk, u, 2, keys) == LR_ERR_ARG);
    CHECK(std::string(lr_last_error_string()).find("modulus P is empty") != std::string::npos);
    REFUSED(lr_keygen_relin_keys(no_p, sk, 1, u, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_rotation_keys_device(no_p, sk, g, 2, u, keys) == LR_ERR_ARG);
    OK(lr_keygen_secret_key(no_p, u, u, 2, skq));                                    // ... which serves the secret and the public key over Q
    count += 3;
    // NULL arguments
    REFUSED(lr_keygen_secret_key(nullptr, u, u, 2, sk2) == LR_ERR_ARG);
    REFUSED(lr_keygen_secret_key(kg, nullptr, u, 2, sk2) == LR_ERR_ARG);
    REFUSED(lr_keygen_secret_key_device(kg, u, nullptr, 2, sk2) == LR_ERR_ARG);
    REFUSED(lr_keygen_secret_key(kg, u, u, 2, nullptr) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key(kg, nullptr, u, 2, pk0, pk1) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key_device(kg, sk, nullptr, 2, pk0, pk1) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key(kg, sk, u, 2, nullptr, pk1) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key(kg, sk, u, 2, pk0, nullptr) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, nullptr, sk, u, 2, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, sk, nullptr, u, 2, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys_device(kg, sk, sk, nullptr, 2, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 2, nullptr) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 2, with_null) == LR_ERR_ARG);
    REFUSED(lr_keygen_relin_keys(kg, nullptr, 2, u, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_relin_keys_device(kg, sk, 2, nullptr, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_rotation_keys(kg, sk, nullptr, 2, u, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_rotation_keys_device(kg, sk, g, 2, u, nullptr) == LR_ERR_ARG);
    count += 17;
    // a poly of another context, an output that is an input or another output, an even Galois element
    REFUSED(lr_keygen_secret_key(kg, u, u, 2, foreign) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key(kg, foreign1, u, 2, pk0, pk1) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key(kg, sk, u, 2, foreign, pk1) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key(kg, sk, u, 2, pk0, foreign) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key(kg, sk, u, 2, pk0, pk0) == LR_ERR_ARG);
    REFUSED(lr_keygen_public_key(kg, sk2, u, 2, sk2, pk1) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, foreign1, sk, u, 2, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, sk, foreign1, u, 2, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 2, with_foreign) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 2, same) == LR_ERR_ARG);
    REFUSED(lr_keygen_switching_keys(kg, inside, sk, u, 1, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_relin_keys(kg, inside, 1, u, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_rotation_keys(kg, sk, even, 2, u, keys) == LR_ERR_ARG);
    REFUSED(lr_keygen_rotation_keys_device(kg, sk, zero, 2, u, keys) == LR_ERR_ARG);
    count += 14;
    // counts, batches and limbs
    REFUSED(lr_keygen_secret_key(kg, u, u, 0, sk2) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_secret_key(kg, u, u, 3, sk3) == LR_ERR_SHAPE);                   // above max_batch
    REFUSED(lr_keygen_secret_key(kg, u, u, 1, sk2) == LR_ERR_SHAPE);                   // differs from the poly's
    REFUSED(lr_keygen_secret_key(kg, u, u, 2, narrow) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_public_key(kg, sk, u, -1, pk0, pk1) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_public_key(kg, sk3, u, 2, pk0, pk1) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_public_key(kg, sk, u, 2, pk0, sk) == LR_ERR_SHAPE);              // pk1 of batch 1
    REFUSED(lr_keygen_public_key(kg, narrow1, u, 2, pk0, pk1) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_public_key(kg, sk, u, 2, narrow, pk1) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 0, keys) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 3, three) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_switching_keys(kg, sk3, sk, u, 2, keys) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_switching_keys(kg, sk, narrow1, u, 2, keys) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 2, with_narrow) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 2, with_batch) == LR_ERR_SHAPE);   // a key whose batch is not 2 beta
    REFUSED(lr_keygen_relin_keys(kg, sk, 3, u, three) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_relin_keys(kg, sk2, 2, u, keys) == LR_ERR_SHAPE);                // one secret key
    REFUSED(lr_keygen_rotation_keys(kg, sk, g, -1, u, keys) == LR_ERR_SHAPE);
    REFUSED(lr_keygen_rotation_keys(kg, sk2, g, 2, u, keys) == LR_ERR_SHAPE);
    count += 19;
    {   // the two contexts on different streams: every entry point of a handle with a ctxP refuses
        hipStream_t st = nullptr;
        CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
        OK(lr_context_set_stream(r.q, st));
        REFUSED(lr_keygen_secret_key(kg, u, u, 2, sk2) == LR_ERR_ARG);
        CHECK(std::string(lr_last_error_string()).find("different streams") != std::string::npos);
        REFUSED(lr_keygen_public_key_device(kg, sk, u, 2, pk0, pk1) == LR_ERR_ARG);
        REFUSED(lr_keygen_switching_keys(kg, sk, sk, u, 2, keys) == LR_ERR_ARG);
        REFUSED(lr_keygen_relin_keys_device(kg, sk, 2, u, keys) == LR_ERR_ARG);
        REFUSED(lr_keygen_rotation_keys(kg, sk, g, 2, u, keys) == LR_ERR_ARG);
        OK(lr_keygen_secret_key(no_p, u, u, 2, skq));                                // a handle without ctxP has one stream
        OK(lr_context_sync(r.q));
        OK(lr_context_set_stream(r.q, nullptr));
        CHECK(hipStreamDestroy(st) == hipSuccess);
        count += 5;
    }
    CHECK(lr::g_stub_launches.load() + lr::g_ckks_expand_launches.load() - before == 4);      // only the two accepted calls launched anything: expansion, transform
    OK(lr_keygen_rotation_keys(kg, sk, g, 2, u, keys));                              // the handle stays usable
    for (lr_poly *p : {sk, sk2, sk3, pk0, pk1, foreign, foreign1, narrow, narrow1, k0, k1, k2, kf, kn, kb, skq, inside}) lr_poly_free(p);
    OK(lr_keygen_destroy(no_p));
    OK(lr_keygen_destroy(kg));
    OK(lr_keygen_destroy(nullptr));
    OK(lr_context_destroy(dev1));
    OK(lr_context_destroy(big));
    OK(lr_context_destroy(small));
    return count;
}

int main() {
    int calls = 0, refused = 0;
    lr_options call_by_call;
    OK(lr_options_init(&call_by_call));
    call_by_call.no_epilogue = 1;
    for (uint64_t N : {(uint64_t)1 << 4, (uint64_t)1 << 12}) {
        calls += exercise(N, 3, 1, nullptr);
        calls += exercise(N, 3, 2, &call_by_call);        // ragged: the last digit owns one row
    }
    calls += exercise(1 << 4, 3, 2, nullptr);
    calls += exercise(1 << 4, 3, 1, &call_by_call);
    calls += exercise(1 << 4, 3, 2, nullptr, 70);         // 70 keys: passes of 32, 32 and 6
    calls += exercise(1 << 4, 3, 1, &call_by_call, 70);
    sequences();
    refused += refusals();
    {   // two handles on two threads, each with its own contexts: nothing is shared but the library's globals
        std::atomic<int> threaded{0};
        std::thread a([&] { threaded += exercise(1 << 12, 3, 2, nullptr); });
        std::thread b([&] { threaded += exercise(1 << 4, 3, 1, &call_by_call); });
        a.join();
        b.join();
        calls += threaded.load();
    }
    return driver_end(ALLOCATIONS | EVENTS | LOG, refused, "keygen: calls %d, refusals %d", calls, refused);
}
