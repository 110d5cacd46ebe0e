// The BFV encryptor's and decryptor's host side under AddressSanitizer + UBSan and under ThreadSanitizer
// (tests/test_host_bfv_encryptor_sanitizers.py): the REAL host code -- lr_bfv_encryptor.cpp with every other host unit of the library --
// compiled with g++ against the host-only HIP stand-in and the launch stand-ins of tests/cpp/hipstub/, which touch the first and the last
// byte of everything a kernel would read or write. pk and sk, fast and through P, host and device-pointer randomness, both shapes
// (lr_options::no_epilogue), batches 1, 3 and max_batch with the pools and the staging buffer reused across calls, wide polys, shared and
// per-ciphertext keys; Decrypt at degrees 0, 1, 2 and 9; two handles on two threads; the recorded launch sequence of both shapes for pk
// through P; every refusal.
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
extern std::atomic<unsigned long long> g_stub_launches, g_encryptor_stub_launches;
void encryptor_stub_clear();
int encryptor_stub_count();
const char *encryptor_stub_name(int i);
unsigned long long encryptor_stub_shared_before(int i);
int encryptor_stub_limbs(int i);
int encryptor_stub_batch(int i);
}  // namespace lr

static const int NQ = 3, NP = 1, MAXB = 5;

static unsigned long long launches() { return lr::g_stub_launches.load() + lr::g_encryptor_stub_launches.load(); }

// one encryptor and one decryptor through every call shape; returns the number of accepted calls
static int exercise(uint64_t N, const lr_options *opt) {
    Rings r(N, Qm, NQ, NP, opt);
    lr_bfv_encryptor *enc = nullptr;
    lr_bfv_decryptor *dec = nullptr;
    OK(opt ? lr_bfv_encryptor_create_ex(r.q, r.p, MAXB, opt, &enc) : lr_bfv_encryptor_create(r.q, r.p, MAXB, &enc));
    OK(lr_bfv_decryptor_create(r.q, MAXB, &dec));
    if (!enc || !dec) return 0;
    int calls = 0;
    for (int round = 0; round < 2; ++round)                                   // the second round reuses the pools and the staging buffer
        for (int batch : {1, 3, MAXB}) {
            const bool wide = (batch + round) % 2 == 1;                       // polys with one limb more than needed: another stride
            const int kb = round == 0 ? 1 : batch;                            // keys and plaintext: one for the batch, or one each
            lr_poly *pk0 = poly(r.q, NQ + NP + (wide ? 1 : 0), kb), *pk1 = poly(r.q, NQ + NP, kb), *sk = poly(r.q, NQ + NP, kb);
            lr_poly *crp = poly(r.q, NQ + NP, batch), *pt = poly(r.q, NQ, kb);
            lr_poly *c0 = poly(r.q, wide ? NQ + 1 : NQ, batch), *c1 = poly(r.q, NQ, batch);
            // exactly [batch][N / 8] and [batch][N] bytes
            std::vector<uint8_t> uc((size_t)batch * N / 8, 0xAA), us((size_t)batch * N / 8, 0xCC), e0((size_t)batch * N, 0x93), e1((size_t)batch * N, 0);
            void *duc = nullptr, *dus = nullptr, *de0 = nullptr, *de1 = nullptr;
            CHECK(hipMalloc(&duc, uc.size()) == hipSuccess && hipMalloc(&dus, us.size()) == hipSuccess);
            CHECK(hipMalloc(&de0, e0.size()) == hipSuccess && hipMalloc(&de1, e1.size()) == hipSuccess);
            for (int fast : {0, 1}) {
                const unsigned long long before = launches();
                OK(lr_bfv_encrypt_pk(enc, fast, pk0, pk1, uc.data(), us.data(), e0.data(), e1.data(), pt, batch, c0, c1));
                OK(lr_bfv_encrypt_sk(enc, fast, sk, crp, e0.data(), pt, batch, c0, c1));
                OK(lr_bfv_encrypt_pk_device(enc, fast, pk0, pk1, duc, dus, de0, de1, pt, batch, c0, c1));
                OK(lr_bfv_encrypt_sk_device(enc, fast, sk, crp, de1, pt, batch, c0, c1));
                CHECK(launches() - before >= 4 * 4);
                calls += 4;
            }
            for (int degree : {0, 1, 2, 9}) {
                std::vector<lr_poly *> ct;
                for (int i = 0; i <= degree; ++i) ct.push_back(poly(r.q, NQ, batch));
                OK(lr_bfv_decrypt(dec, ct.data(), degree, sk, c1, batch));
                OK(lr_bfv_decrypt(dec, ct.data(), degree, sk, ct[degree], batch));           // pt_out is the top component
                calls += 2;
                for (lr_poly *p : ct) lr_poly_free(p);
            }
            OK(lr_context_sync(r.q));
            for (void *p : {duc, dus, de0, de1}) (void)hipFree(p);
            for (lr_poly *p : {pk0, pk1, sk, crp, pt, c0, c1}) lr_poly_free(p);
        }
    OK(lr_bfv_decryptor_destroy(dec));
    OK(lr_bfv_encryptor_destroy(enc));
    return calls;
}

// pk through P at N = 2^4, where a transform is one launch: the encryptor's own launches with the count of shared launches (transforms,
// coefficient-wise calls, the ModDown) between them
static void sequences() {
    const uint64_t N = 16;
    const int batch = 2;
    for (int call_by_call : {0, 1}) {
        lr_options opt;
        OK(lr_options_init(&opt));
        opt.no_epilogue = call_by_call;
        Rings r(N, Qm, NQ, NP, &opt);
        lr_bfv_encryptor *enc = nullptr;
        OK(lr_bfv_encryptor_create_ex(r.q, r.p, batch, &opt, &enc));
        lr_poly *pk0 = poly(r.q, NQ + NP, 1), *pk1 = poly(r.q, NQ + NP, 1), *pt = poly(r.q, NQ, 1), *c0 = poly(r.q, NQ, batch), *c1 = poly(r.q, NQ, batch);
        std::vector<uint8_t> bits((size_t)batch * N / 8, 0xFF), noise((size_t)batch * N, 0x80);
        lr::encryptor_stub_clear();
        const unsigned long long s0 = lr::g_stub_launches.load();
        OK(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, bits.data(), bits.data(), noise.data(), noise.data(), pt, batch, c0, c1));
        const unsigned long long total = lr::g_stub_launches.load() - s0;
        auto at = [&](int i) { return lr::encryptor_stub_shared_before(i) - s0; };
        auto is = [&](int i, const char *name, int limbs) {
            return std::string(lr::encryptor_stub_name(i)) == name && lr::encryptor_stub_limbs(i) == limbs && lr::encryptor_stub_batch(i) == batch;
        };
        if (call_by_call) {
            // the reference's order (bfv/encryptor.go:196-222): SampleTernaryMontgomeryNTT = the expansion and NTT over Q and over P; two
            // MulCoeffsMontgomery and two InvNTT, each over Q and over P; Sample + Add twice; two ModDownPQ (extension, subtract-multiply);
            // the Add of the plaintext
            CHECK(lr::encryptor_stub_count() == 3);
            CHECK(is(0, "ternary", NQ + NP) && at(0) == 0);
            CHECK(is(1, "noise_expand", NQ + NP) && at(1) == 2 + 4 + 4);
            CHECK(is(2, "noise_expand", NQ + NP) && at(2) == 2 + 4 + 4 + 2);
            CHECK(total == 2 + 4 + 4 + 2 + 2 + 2 * 2 + 1);
        } else {
            // the expansion, NTT over Q and over P, ONE launch for both products over all of Q||P, InvNTT of both polys over Q and over P,
            // ONE noise launch for both components, two ModDownPQ, the Add of the plaintext
            CHECK(lr::encryptor_stub_count() == 2);
            CHECK(is(0, "ternary", NQ + NP) && at(0) == 0);
            CHECK(is(1, "noise_add2", NQ + NP) && at(1) == 2 + 1 + 2);
            CHECK(total >= 2 + 1 + 2 + 2 + 1 && total <= 2 + 1 + 2 + 2 * 2 + 1);
        }
        for (lr_poly *p : {pk0, pk1, pt, c0, c1}) lr_poly_free(p);
        OK(lr_bfv_encryptor_destroy(enc));
    }
}

static int refusals() {
    const uint64_t N = 16;
    int count = 0;
    Rings r(N, Qm, NQ, NP, nullptr), other(N, Qm, NQ, NP, nullptr);
    lr_context *small = nullptr, *big = nullptr;
    OK(lr_context_create(4, Qm, NQ, 0, &small));
    OK(lr_context_create(2 * N, Qm + NQ, NP, 0, &big));
    lr_context *dev1 = nullptr;
    OK(lr_context_create(N, Qm + NQ, NP, 1, &dev1));
    lr_bfv_encryptor *enc = nullptr, *none = nullptr, *fast_only = nullptr;
    lr_bfv_decryptor *dec = nullptr, *nodec = nullptr;
    const unsigned long long before = launches();
    // creation
    REFUSED(lr_bfv_encryptor_create(nullptr, r.p, 1, &none) == LR_ERR_ARG);
    REFUSED(lr_bfv_encryptor_create(r.q, r.p, 1, nullptr) == LR_ERR_ARG);
    REFUSED(lr_bfv_encryptor_create(r.q, r.p, 0, &none) == LR_ERR_ARG && none == nullptr);
    REFUSED(lr_bfv_encryptor_create(r.q, r.p, 65536, &none) == LR_ERR_ARG);
    REFUSED(lr_bfv_encryptor_create(small, nullptr, 1, &none) == LR_ERR_ARG);                 // N < 8
    REFUSED(lr_bfv_encryptor_create(r.q, big, 1, &none) == LR_ERR_ARG);                       // ctxP with another N
    REFUSED(lr_bfv_encryptor_create(r.q, dev1, 1, &none) == LR_ERR_ARG);                      // ctxP on another device
    lr_options bad;
    OK(lr_options_init(&bad));
    bad.version = 99;
    REFUSED(lr_bfv_encryptor_create_ex(r.q, r.p, 1, &bad, &none) == LR_ERR_ARG);
    REFUSED(lr_bfv_decryptor_create(nullptr, 1, &nodec) == LR_ERR_ARG);
    REFUSED(lr_bfv_decryptor_create(r.q, 1, nullptr) == LR_ERR_ARG);
    REFUSED(lr_bfv_decryptor_create(r.q, 0, &nodec) == LR_ERR_ARG);
    REFUSED(lr_bfv_decryptor_create(r.q, 65536, &nodec) == LR_ERR_ARG);
    count += 12;
    OK(lr_bfv_encryptor_create(r.q, r.p, 2, &enc));
    OK(lr_bfv_encryptor_create(r.q, nullptr, 2, &fast_only));
    OK(lr_bfv_decryptor_create(r.q, 2, &dec));
    lr_poly *pk0 = poly(r.q, NQ + NP, 1), *pk1 = poly(r.q, NQ + NP, 1), *sk = poly(r.q, NQ + NP, 1), *crp = poly(r.q, NQ + NP, 2), *pt = poly(r.q, NQ, 2);
    lr_poly *c0 = poly(r.q, NQ, 2), *c1 = poly(r.q, NQ, 2), *foreign = poly(other.q, NQ + NP, 2), *narrow = poly(r.q, NQ - 1, 2), *three = poly(r.q, NQ + NP, 3);
    lr_poly *keyq = poly(r.q, NQ, 1);
    std::vector<uint8_t> b((size_t)3 * N, 0);
    const uint8_t *u = b.data();
    // the form against the handle
    REFUSED(lr_bfv_encrypt_pk(fast_only, 0, pk0, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    CHECK(std::string(lr_last_error_string()).find("fast form") != std::string::npos);
    REFUSED(lr_bfv_encrypt_sk(fast_only, 0, sk, crp, u, pt, 2, c0, c1) == LR_ERR_ARG);
    OK(lr_bfv_encrypt_pk(fast_only, 1, keyq, keyq, u, u, u, u, pt, 2, c0, c1));               // ... which serves the fast forms, keys over Q
    // NULL arguments
    REFUSED(lr_bfv_encrypt_pk(nullptr, 0, pk0, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_pk(enc, 0, nullptr, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, nullptr, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, nullptr, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_pk_device(enc, 0, pk0, pk1, u, nullptr, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, u, nullptr, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, u, pt, 2, c0, nullptr) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_sk(enc, 0, nullptr, crp, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_sk(enc, 0, sk, nullptr, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_sk(enc, 0, sk, crp, nullptr, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_sk_device(enc, 0, sk, crp, nullptr, pt, 2, c0, c1) == LR_ERR_ARG);
    // out_c0 == out_c1, a poly of another context
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, u, pt, 2, c0, c0) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_sk(enc, 1, sk, crp, u, pt, 2, c1, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_pk(enc, 0, foreign, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, u, foreign, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_sk(enc, 0, sk, foreign, u, pt, 2, c0, c1) == LR_ERR_ARG);
    REFUSED(lr_bfv_encrypt_sk(enc, 0, sk, crp, u, pt, 2, foreign, c1) == LR_ERR_ARG);
    // batch and limbs
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, u, pt, 0, c0, c1) == LR_ERR_SHAPE);
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, u, three, 3, three, c1) == LR_ERR_SHAPE);   // above max_batch
    REFUSED(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, u, pt, 1, c0, c1) == LR_ERR_SHAPE);         // differs from the polys'
    REFUSED(lr_bfv_encrypt_pk(enc, 0, three, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_SHAPE);
    REFUSED(lr_bfv_encrypt_sk(enc, 0, sk, pk0, u, pt, 2, c0, c1) == LR_ERR_SHAPE);                   // crp of batch 1
    REFUSED(lr_bfv_encrypt_pk(enc, 0, keyq, pk1, u, u, u, u, pt, 2, c0, c1) == LR_ERR_SHAPE);        // a key over Q for the form through P
    REFUSED(lr_bfv_encrypt_pk(enc, 1, pk0, pk1, u, u, u, u, pt, 2, narrow, c1) == LR_ERR_SHAPE);
    REFUSED(lr_bfv_encrypt_sk(enc, 1, sk, crp, u, narrow, 2, c0, c1) == LR_ERR_SHAPE);
    // decrypt
    const lr_poly *ct[2] = {c0, c1}, *with_null[2] = {c0, nullptr}, *with_foreign[2] = {c0, foreign}, *with_narrow[2] = {narrow, c1};
    REFUSED(lr_bfv_decrypt(dec, ct, -1, sk, pt, 2) == LR_ERR_ARG);
    REFUSED(lr_bfv_decrypt(nullptr, ct, 1, sk, pt, 2) == LR_ERR_ARG);
    REFUSED(lr_bfv_decrypt(dec, nullptr, 1, sk, pt, 2) == LR_ERR_ARG);
    REFUSED(lr_bfv_decrypt(dec, ct, 1, nullptr, pt, 2) == LR_ERR_ARG);
    REFUSED(lr_bfv_decrypt(dec, ct, 1, sk, nullptr, 2) == LR_ERR_ARG);
    REFUSED(lr_bfv_decrypt(dec, with_null, 1, sk, pt, 2) == LR_ERR_ARG);
    REFUSED(lr_bfv_decrypt(dec, with_foreign, 1, sk, pt, 2) == LR_ERR_ARG);
    REFUSED(lr_bfv_decrypt(dec, ct, 1, foreign, pt, 2) == LR_ERR_ARG);
    REFUSED(lr_bfv_decrypt(dec, ct, 1, sk, pt, 0) == LR_ERR_SHAPE);
    REFUSED(lr_bfv_decrypt(dec, ct, 1, sk, pt, 3) == LR_ERR_SHAPE);
    REFUSED(lr_bfv_decrypt(dec, ct, 1, sk, pt, 1) == LR_ERR_SHAPE);
    REFUSED(lr_bfv_decrypt(dec, with_narrow, 1, sk, pt, 2) == LR_ERR_SHAPE);
    REFUSED(lr_bfv_decrypt(dec, ct, 1, narrow, pt, 2) == LR_ERR_SHAPE);
    count += 2 + 11 + 6 + 8 + 13;
    CHECK(launches() - before == 5);                                                               // only the one accepted call launched anything
    OK(lr_bfv_encrypt_pk(enc, 0, pk0, pk1, u, u, u, u, pt, 2, c0, c1));                            // the handles stay usable
    OK(lr_bfv_decrypt(dec, ct, 1, sk, pt, 2));
    for (lr_poly *p : {pk0, pk1, sk, crp, pt, c0, c1, foreign, narrow, three, keyq}) lr_poly_free(p);
    OK(lr_bfv_decryptor_destroy(dec));
    OK(lr_bfv_encryptor_destroy(fast_only));
    OK(lr_bfv_encryptor_destroy(enc));
    OK(lr_bfv_encryptor_destroy(nullptr));
    OK(lr_bfv_decryptor_destroy(nullptr));
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
        calls += exercise(N, nullptr);
        calls += exercise(N, &call_by_call);
    }
    sequences();
    refused += refusals();
    {   // two handles on two threads, each with its own contexts: nothing is shared but the library's globals
        std::atomic<int> threaded{0};
        std::thread a([&] { threaded += exercise(1 << 12, nullptr); });
        std::thread b([&] { threaded += exercise(1 << 4, &call_by_call); });
        a.join();
        b.join();
        calls += threaded.load();
    }
    return driver_end(ALLOCATIONS | EVENTS | LOG, refused, "bfv_encryptor: calls %d, refusals %d", calls, refused);
}
