// The collective handle's host side under AddressSanitizer + UBSan and under ThreadSanitizer (tests/test_host_collective_sanitizers.py):
// the REAL host code -- lr_collective.cpp with every other host unit of the library -- compiled with g++ against the host-only HIP stand-in
// and the launch stand-ins of tests/cpp/hipstub/, which touch the first and the last byte of everything a kernel would read or write. Every
// entry point in its host and device-pointer form, both shapes (lr_options::no_epilogue), batches 1, 3 and max_batch with the pool and the
// staging buffer reused across consecutive host-form calls, wide polys, shared and per-ciphertext keys, |P| = 1 and |P| = 2, every level,
// 33 shares (a second fold pass) with out aliasing a share and the base; two handles on two threads; the launch counts of both shapes;
// every refusal.
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
extern std::atomic<unsigned long long> g_stub_launches, g_encryptor_stub_launches, g_ckks_expand_launches, g_ckks_fast_launches, g_cks_share_launches,
    g_pcks_addend_launches, g_fold_launches;
}  // namespace lr

static const int MAXB = 5, SHARES = 33;

// one handle through every entry point; returns the number of accepted calls
static int exercise(uint64_t N, int nq, int np, const lr_options *opt) {
    Rings r(N, Qm, nq, np, opt);
    const int rows = nq + np;
    lr_collective *col = nullptr;
    OK(opt ? lr_collective_create_ex(r.q, r.p, MAXB, opt, &col) : lr_collective_create(r.q, r.p, MAXB, &col));
    if (!col) return 0;
    int calls = 0;
    for (int round = 0; round < 2; ++round)                                   // the second round reuses the pool and the staging buffer
        for (int n : {1, 3, MAXB}) {
            const bool wide = (n + round) % 2 == 1;                           // polys with one limb more than needed: another stride
            const int kb = round == 0 ? 1 : n;                                // keys: one for the call, or one per ciphertext
            const int level = (n + round) % nq;                               // every level over the runs
            lr_poly *sk_in = poly(r.q, wide ? nq : rows, kb), *sk_out = poly(r.q, rows, kb), *pk0 = poly(r.q, rows + (wide ? 1 : 0), kb), *pk1 = poly(r.q, rows, kb);
            lr_poly *c1 = poly(r.q, nq + (wide ? 1 : 0), n), *o0 = poly(r.q, nq, n), *o1 = poly(r.q, nq + (wide ? 0 : 1), n), *base = poly(r.q, nq, n);
            std::vector<lr_poly *> shares;
            for (int k = 0; k < SHARES; ++k) shares.push_back(poly(r.q, nq + (k % 2), n));
            // exactly [n][N / 8] and [n][N] bytes
            std::vector<uint8_t> bits((size_t)n * N / 8, 0xAA), e((size_t)n * N, 0x93);
            void *dbits = nullptr, *de = nullptr;
            CHECK(hipMalloc(&dbits, bits.size()) == hipSuccess && hipMalloc(&de, e.size()) == hipSuccess);
            // host-form calls one behind the other: each refills the pinned buffer the one before staged through
            OK(lr_collective_ckks_cks_share(col, level, sk_in, sk_out, c1, e.data(), n, o0));
            OK(lr_collective_bfv_cks_share(col, sk_in, sk_out, c1, e.data(), n, o0));
            OK(lr_collective_ckks_pcks_share(col, level, sk_in, pk0, pk1, c1, bits.data(), bits.data(), e.data(), e.data(), n, o0, o1));
            OK(lr_collective_bfv_pcks_share(col, sk_in, pk0, pk1, c1, bits.data(), bits.data(), e.data(), e.data(), n, o0, o1));
            OK(lr_collective_ckks_cks_share_device(col, level, sk_in, sk_out, c1, de, n, o0));
            OK(lr_collective_bfv_cks_share_device(col, sk_in, sk_out, c1, de, n, o0));
            OK(lr_collective_ckks_pcks_share_device(col, level, sk_in, pk0, pk1, c1, dbits, dbits, de, de, n, o0, o1));
            OK(lr_collective_bfv_pcks_share_device(col, sk_in, pk0, pk1, c1, dbits, dbits, de, de, n, o0, o1));
            OK(lr_collective_aggregate(col, level, nullptr, shares.data(), 1, o0));                     // KeySwitch's Copy
            OK(lr_collective_aggregate(col, level, base, shares.data(), SHARES, o0));                   // two passes, the base on the second
            OK(lr_collective_aggregate(col, level, nullptr, shares.data(), SHARES, shares[SHARES - 1]));  // out = a share of the second pass
            OK(lr_collective_aggregate(col, level, base, shares.data(), 3, base));                      // out = the base
            calls += 12;
            OK(lr_context_sync(r.q));
            for (void *p : {dbits, de}) (void)hipFree(p);
            for (lr_poly *p : {sk_in, sk_out, pk0, pk1, c1, o0, o1, base}) lr_poly_free(p);
            for (lr_poly *p : shares) lr_poly_free(p);
        }
    OK(lr_collective_destroy(col));
    return calls;
}

struct Counts {
    unsigned long long stub, enc, expand, fast, share, addend, fold;
};
static Counts snap() {
    return Counts{lr::g_stub_launches.load(),      lr::g_encryptor_stub_launches.load(), lr::g_ckks_expand_launches.load(), lr::g_ckks_fast_launches.load(),
                  lr::g_cks_share_launches.load(), lr::g_pcks_addend_launches.load(),    lr::g_fold_launches.load()};
}
static Counts since(const Counts &a) {
    const Counts b = snap();
    return Counts{b.stub - a.stub, b.enc - a.enc, b.expand - a.expand, b.fast - a.fast, b.share - a.share, b.addend - a.addend, b.fold - a.fold};
}
static bool is(const Counts &d, unsigned long long stub, unsigned long long enc, unsigned long long expand, unsigned long long fast, unsigned long long share,
               unsigned long long addend, unsigned long long fold, const char *what, int shape) {
    std::printf("launches %-16s %s: shared %llu, encryptor kernels %llu (expansions %llu, pk passes %llu), share %llu, addend %llu, fold %llu\n", what,
                shape ? "call by call" : "default", d.stub, d.enc, d.expand, d.fast, d.share, d.addend, d.fold);
    return d.stub == stub && d.enc == enc && d.expand == expand && d.fast == fast && d.share == share && d.addend == addend && d.fold == fold;
}

// at N = 2^4 a transform is one launch per context.  md / md_ntt: what one ModDownSplitedPQ / ModDownSplitedNTTPQ of the same contexts
// launches (the second with its inverse transform of the rows of P), measured here through the basis extender's own entry points
static void sequences() {
    const uint64_t N = 16;
    const int nq = 3, np = 2, n = 3, top = nq - 1;
    for (int cbc : {0, 1}) {
        lr_options opt;
        OK(lr_options_init(&opt));
        opt.no_epilogue = cbc;
        Rings r(N, Qm, nq, np, &opt);
        lr_collective *col = nullptr;
        lr_bext *bext = nullptr;
        OK(lr_collective_create_ex(r.q, r.p, n, &opt, &col));
        OK(lr_bext_create(r.q, r.p, &bext));
        lr_poly *sk = poly(r.q, nq + np, 1), *sk2 = poly(r.q, nq + np, 1), *pk0 = poly(r.q, nq + np, 1), *pk1 = poly(r.q, nq + np, 1);
        lr_poly *c1 = poly(r.q, nq, n), *o0 = poly(r.q, nq, n), *o1 = poly(r.q, nq, n), *hp = poly(r.p, np, n);
        std::vector<lr_poly *> shares;
        for (int k = 0; k < SHARES; ++k) shares.push_back(poly(r.q, nq, n));
        std::vector<uint8_t> e((size_t)n * N, 0x80), bits((size_t)n * N / 8, 0x55);
        Counts s = snap();
        OK(lr_moddown_split_pq(bext, top, c1, hp, o0));
        const unsigned long long md = since(s).stub;
        s = snap();
        OK(lr_moddown_split_ntt_pq(bext, top, c1, hp, o0));
        const unsigned long long md_ntt = since(s).stub;
        s = snap();
        OK(lr_moddown_split_ntt_pq(bext, 0, c1, hp, o0));
        const unsigned long long md_ntt0 = since(s).stub;
        std::printf("launches of one ModDownSplitedPQ %llu, of one ModDownSplitedNTTPQ %llu, at level 0 %llu (%s)\n", md, md_ntt, md_ntt0,
                    cbc ? "call by call" : "default");
        CHECK(md >= 1 && md_ntt >= 2 && md_ntt0 >= 2);
        // CKKS CKS
        s = snap();
        OK(lr_collective_ckks_cks_share(col, top, sk, sk2, c1, e.data(), n, o0));
        if (cbc) CHECK(is(since(s), 6 + md_ntt, 1, 1, 0, 0, 0, 0, "ckks cks", cbc));      // Sub, Mul, MulScalarBigint, NTT (Q, P), Add, then the ModDown with its InvNTT
        else CHECK(is(since(s), 1 + (md_ntt - 1), 1, 1, 0, 1, 0, 0, "ckks cks", cbc));    // expansion, NTT (Q), the share pass, the ModDown without its InvNTT
        s = snap();
        OK(lr_collective_ckks_cks_share(col, 0, sk, sk2, c1, e.data(), n, o0));
        if (cbc) CHECK(is(since(s), 6 + md_ntt0, 1, 1, 0, 0, 0, 0, "ckks cks level 0", cbc));
        else CHECK(is(since(s), 1 + (md_ntt0 - 1), 2, 2, 0, 1, 0, 0, "ckks cks level 0", cbc));   // below the top level the rows of Q and of P expand apart
        // BFV CKS
        s = snap();
        OK(lr_collective_bfv_cks_share(col, sk, sk2, c1, e.data(), n, o0));
        if (cbc) CHECK(is(since(s), 6 + md, 1, 0, 0, 0, 0, 0, "bfv cks", cbc));           // NTT, Sub, Mul, MulScalarBigint, InvNTT, Add; Sample is one expansion
        else CHECK(is(since(s), 2 + md, 2, 1, 0, 1, 0, 0, "bfv cks", cbc));               // NTT, the share pass, InvNTT, noise on Q, residues on P, ModDown
        // CKKS PCKS
        s = snap();
        OK(lr_collective_ckks_pcks_share(col, top, sk, pk0, pk1, c1, bits.data(), bits.data(), e.data(), e.data(), n, o0, o1));
        if (cbc) CHECK(is(since(s), 15 + 2 * md_ntt, 3, 2, 0, 0, 0, 0, "ckks pcks", cbc));
        else CHECK(is(since(s), 3 + 2 * (md_ntt - 1), 2, 1, 1, 0, 1, 0, "ckks pcks", cbc));   // one expansion, NTT (Q, P), one pk pass, InvNTT (P) of both, two ModDowns, the addend
        // BFV PCKS
        s = snap();
        OK(lr_collective_bfv_pcks_share(col, sk, pk0, pk1, c1, bits.data(), bits.data(), e.data(), e.data(), n, o0, o1));
        if (cbc) CHECK(is(since(s), 18 + 2 * md, 3, 0, 0, 0, 0, 0, "bfv pcks", cbc));
        else CHECK(is(since(s), 9 + 2 * md, 2, 0, 0, 0, 0, 0, "bfv pcks", cbc));          // NTT (Q, P), mul2, InvNTT (Q, P), two ModDowns, NTT, Mul, InvNTT, Add
        // the fold: 33 shares and a base
        s = snap();
        OK(lr_collective_aggregate(col, top, c1, shares.data(), SHARES, o0));
        if (cbc) CHECK(is(since(s), SHARES, 0, 0, 0, 0, 0, 0, "fold 33 + base", cbc));    // 32 Add calls, then KeySwitch's
        else CHECK(is(since(s), 0, 0, 0, 0, 0, 0, 2, "fold 33 + base", cbc));
        s = snap();
        OK(lr_collective_aggregate(col, top, nullptr, shares.data(), 1, o0));
        if (cbc) CHECK(is(since(s), 1, 0, 0, 0, 0, 0, 0, "fold 1 (Copy)", cbc));
        else CHECK(is(since(s), 0, 0, 0, 0, 0, 0, 1, "fold 1 (Copy)", cbc));
        for (lr_poly *p : {sk, sk2, pk0, pk1, c1, o0, o1, hp}) lr_poly_free(p);
        for (lr_poly *p : shares) lr_poly_free(p);
        OK(lr_bext_destroy(bext));
        OK(lr_collective_destroy(col));
    }
}

static int refusals() {
    const uint64_t N = 16;
    const int nq = 3, np = 1, rows = 4, top = 2;
    int count = 0;
    Rings r(N, Qm, nq, np, nullptr), other(N, Qm, nq, np, nullptr);
    lr_context *small = nullptr, *smallp = nullptr, *big = nullptr, *dev1 = nullptr;
    OK(lr_context_create(4, Qm, nq, 0, &small));
    OK(lr_context_create(4, Qm + nq, np, 0, &smallp));
    OK(lr_context_create(2 * N, Qm + nq, np, 0, &big));
    OK(lr_context_create(N, Qm + nq, np, 1, &dev1));
    lr_collective *col = nullptr, *none = nullptr;
    const Counts before = snap();
    // creation
    REFUSED(lr_collective_create(nullptr, r.p, 1, &none) == LR_ERR_ARG);
    REFUSED(lr_collective_create(r.q, r.p, 1, nullptr) == LR_ERR_ARG);
    REFUSED(lr_collective_create(r.q, nullptr, 1, &none) == LR_ERR_ARG && none == nullptr);   // ctxP is required
    CHECK(std::string(lr_last_error_string()).find("modulus P is empty") != std::string::npos);
    REFUSED(lr_collective_create(r.q, r.p, 0, &none) == LR_ERR_ARG && none == nullptr);
    REFUSED(lr_collective_create(r.q, r.p, 65536, &none) == LR_ERR_ARG);
    REFUSED(lr_collective_create(small, smallp, 1, &none) == LR_ERR_ARG);                // N < 8
    REFUSED(lr_collective_create(r.q, big, 1, &none) == LR_ERR_ARG);                     // ctxP with another N
    REFUSED(lr_collective_create(r.q, dev1, 1, &none) == LR_ERR_ARG);                    // ctxP on another device
    lr_options bad;
    OK(lr_options_init(&bad));
    bad.version = 99;
    REFUSED(lr_collective_create_ex(r.q, r.p, 1, &bad, &none) == LR_ERR_ARG);
    count += 9;
    OK(lr_collective_create(r.q, r.p, 2, &col));
    lr_poly *sk = poly(r.q, rows, 1), *sk3 = poly(r.q, rows, 3), *pk0 = poly(r.q, rows, 1), *pk1 = poly(r.q, rows, 1), *pkq = poly(r.q, nq, 1);
    lr_poly *c1 = poly(r.q, nq, 2), *c11 = poly(r.q, nq, 1), *c13 = poly(r.q, nq, 3), *o0 = poly(r.q, nq, 2), *o1 = poly(r.q, nq, 2), *o3 = poly(r.q, nq, 3);
    lr_poly *foreign = poly(other.q, nq, 2), *foreign1 = poly(other.q, rows, 1), *narrow = poly(r.q, nq - 1, 2), *narrow1 = poly(r.q, nq - 1, 1);
    lr_poly *s0 = poly(r.q, nq, 2), *s1 = poly(r.q, nq, 2), *s11 = poly(r.q, nq, 1);
    lr_poly *head = nullptr, *inside = nullptr;
    {
        uint64_t *d = nullptr;
        OK(lr_poly_info(o0, nullptr, nullptr, nullptr, (void **)&d));
        OK(lr_poly_wrap(r.q, d, nq, 1, &head));                                         // member 0 of o0
        OK(lr_poly_wrap(r.q, d + N, nq, 1, &inside));                                   // from limb 1 of member 0 on: a partial overlap with head
    }
    const lr_poly *two[2] = {s0, s1}, *with_null[2] = {s0, nullptr}, *with_foreign[2] = {s0, foreign}, *mixed[2] = {s0, s11}, *one3[1] = {o3},
                  *one_inside[1] = {inside}, *one11[1] = {s11};
    std::vector<uint8_t> b((size_t)3 * N, 0);
    const uint8_t *u = b.data();
    // NULL arguments
    REFUSED(lr_collective_ckks_cks_share(nullptr, top, sk, sk, c1, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_cks_share(col, top, nullptr, sk, c1, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_cks_share_device(col, top, sk, nullptr, c1, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, nullptr, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_cks_share_device(col, top, sk, sk, c1, nullptr, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, c1, u, 2, nullptr) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_cks_share(nullptr, sk, sk, c1, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_cks_share_device(col, sk, sk, c1, nullptr, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_cks_share(col, sk, sk, c1, u, 2, nullptr) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share(col, top, nullptr, pk0, pk1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share(col, top, sk, nullptr, pk1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share_device(col, top, sk, pk0, pk1, c1, nullptr, u, u, u, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share_device(col, top, sk, pk0, pk1, c1, u, u, u, nullptr, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share(col, top, sk, pk0, pk1, c1, u, u, u, u, 2, o0, nullptr) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_pcks_share(col, sk, pk0, nullptr, c1, u, u, u, u, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_pcks_share_device(col, sk, pk0, pk1, nullptr, u, u, u, u, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_pcks_share_device(col, sk, pk0, pk1, c1, u, nullptr, u, u, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(nullptr, top, nullptr, two, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(col, top, nullptr, nullptr, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(col, top, nullptr, with_null, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(col, top, nullptr, two, 2, nullptr) == LR_ERR_ARG);
    count += 21;
    // a poly of another context, an output that shares memory with an input or with the other output, a partial overlap in the fold
    REFUSED(lr_collective_ckks_cks_share(col, top, foreign1, sk, c1, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, foreign1, c1, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_cks_share(col, sk, sk, foreign, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_cks_share(col, sk, sk, c1, u, 2, foreign) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, c1, u, 2, c1) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_cks_share_device(col, o0, sk, c1, u, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, head, u, 1, inside) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share(col, top, foreign1, pk0, pk1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share(col, top, sk, pk0, foreign1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_pcks_share(col, sk, pk0, pk1, c1, u, u, u, u, 2, o0, foreign) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_pcks_share(col, sk, pk0, pk1, c1, u, u, u, u, 2, o0, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share_device(col, top, sk, pk0, pk1, c1, u, u, u, u, 2, c1, o1) == LR_ERR_ARG);
    REFUSED(lr_collective_ckks_pcks_share(col, top, sk, pk0, pk1, c1, u, u, u, u, 2, o0, c1) == LR_ERR_ARG);
    REFUSED(lr_collective_bfv_pcks_share(col, sk, pk0, pk1, c11, u, u, u, u, 1, head, inside) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(col, top, nullptr, with_foreign, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(col, top, foreign, two, 2, o0) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(col, top, nullptr, two, 2, foreign) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(col, top, nullptr, one_inside, 1, head) == LR_ERR_ARG);
    REFUSED(lr_collective_aggregate(col, top, inside, one11, 1, head) == LR_ERR_ARG);
    count += 19;
    // levels, batches and limbs
    REFUSED(lr_collective_ckks_cks_share(col, nq, sk, sk, c1, u, 2, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_ckks_cks_share(col, -1, sk, sk, c1, u, 2, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, c1, u, 0, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, c13, u, 3, o3) == LR_ERR_SHAPE);      // above max_batch
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, c1, u, 1, o0) == LR_ERR_SHAPE);       // differs from the polys'
    REFUSED(lr_collective_ckks_cks_share(col, top, sk3, sk, c1, u, 2, o0) == LR_ERR_SHAPE);      // keys: batch 1 or the call's
    REFUSED(lr_collective_ckks_cks_share(col, top, narrow1, sk, c1, u, 2, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, c11, u, 2, o0) == LR_ERR_SHAPE);      // c1 of batch 1
    REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, c1, u, 2, narrow) == LR_ERR_SHAPE);
    OK(lr_collective_ckks_cks_share(col, top - 1, sk, sk, narrow, u, 2, o0));                  // ... which is enough one level down
    REFUSED(lr_collective_bfv_cks_share(col, sk, sk, narrow, u, 2, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_bfv_cks_share(col, sk, sk, c1, u, -1, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_ckks_pcks_share(col, nq, sk, pk0, pk1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_SHAPE);
    REFUSED(lr_collective_ckks_pcks_share(col, top, sk, pkq, pk1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_SHAPE);   // the public key over Q only
    REFUSED(lr_collective_ckks_pcks_share(col, top, sk, pk0, pk1, c1, u, u, u, u, 2, o0, narrow) == LR_ERR_SHAPE);
    REFUSED(lr_collective_bfv_pcks_share(col, sk, pk0, pkq, c1, u, u, u, u, 2, o0, o1) == LR_ERR_SHAPE);
    REFUSED(lr_collective_bfv_pcks_share(col, sk, pk0, pk1, c1, u, u, u, u, 0, o0, o1) == LR_ERR_SHAPE);
    REFUSED(lr_collective_bfv_pcks_share(col, sk3, pk0, pk1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_SHAPE);
    REFUSED(lr_collective_aggregate(col, top, nullptr, two, 0, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_aggregate(col, nq, nullptr, two, 2, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_aggregate(col, top, nullptr, mixed, 2, o0) == LR_ERR_SHAPE);           // every poly has the same batch
    REFUSED(lr_collective_aggregate(col, top, c11, two, 2, o0) == LR_ERR_SHAPE);
    REFUSED(lr_collective_aggregate(col, top, nullptr, two, 2, narrow) == LR_ERR_SHAPE);
    REFUSED(lr_collective_aggregate(col, top, nullptr, one3, 1, o3) == LR_ERR_SHAPE);            // above max_batch
    count += 23;
    {   // the two contexts on different streams: every entry point refuses, and so does creation
        hipStream_t st = nullptr;
        CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
        OK(lr_context_set_stream(r.q, st));
        REFUSED(lr_collective_ckks_cks_share(col, top, sk, sk, c1, u, 2, o0) == LR_ERR_ARG);
        CHECK(std::string(lr_last_error_string()).find("different streams") != std::string::npos);
        REFUSED(lr_collective_bfv_cks_share_device(col, sk, sk, c1, u, 2, o0) == LR_ERR_ARG);
        REFUSED(lr_collective_ckks_pcks_share(col, top, sk, pk0, pk1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_ARG);
        REFUSED(lr_collective_bfv_pcks_share_device(col, sk, pk0, pk1, c1, u, u, u, u, 2, o0, o1) == LR_ERR_ARG);
        REFUSED(lr_collective_aggregate(col, top, nullptr, two, 2, o0) == LR_ERR_ARG);
        REFUSED(lr_collective_create(r.q, r.p, 1, &none) == LR_ERR_ARG && none == nullptr);
        OK(lr_context_sync(r.q));
        OK(lr_context_set_stream(r.q, nullptr));
        CHECK(hipStreamDestroy(st) == hipSuccess);
        count += 6;
    }
    {   // only the one accepted call launched anything
        const Counts d = since(before);
        CHECK(d.share == 1 && d.expand == 2 && d.fold == 0 && d.addend == 0 && d.fast == 0);
    }
    OK(lr_collective_aggregate(col, top, o1, two, 2, o1));                               // the handle stays usable
    for (lr_poly *p : {sk, sk3, pk0, pk1, pkq, c1, c11, c13, o0, o1, o3, foreign, foreign1, narrow, narrow1, s0, s1, s11, head, inside}) lr_poly_free(p);
    OK(lr_collective_destroy(col));
    OK(lr_collective_destroy(nullptr));
    OK(lr_context_destroy(dev1));
    OK(lr_context_destroy(big));
    OK(lr_context_destroy(smallp));
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
        calls += exercise(N, 3, 2, &call_by_call);
    }
    calls += exercise(1 << 4, 3, 2, nullptr);
    calls += exercise(1 << 4, 3, 1, &call_by_call);
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
    return driver_end(ALLOCATIONS | EVENTS | LOG, refused, "collective: calls %d, refusals %d", calls, refused);
}
