// What the drivers under tests/cpp share: the check macros with their counters, both refusal forms and the refusal log, the prime tables,
// the poly allocator, the Q and P contexts of a handle, and the tail of main.  TEST INFRASTRUCTURE.
#pragma once
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "lattigo_ring.h"

namespace lr {
extern std::atomic<unsigned long long> g_stub_launches, g_lincomb_launches, g_combine_launches;      // every counter of stub_launch.cpp's launches
}

static std::atomic<int> g_fail{0}, g_calls{0}, g_refusals{0};
#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            std::fprintf(stderr, "CHECK failed: %s (line %d): %s\n", #cond, __LINE__, lr_last_error_string()); \
            ++g_fail;                                                                                            \
        }                                                                                                        \
    } while (0)
#define OK(x) CHECK((x) == LR_OK)
// (a driver that asks more of a successful call defines its own RUN before it includes this header)
#ifndef RUN
#define RUN(x)       \
    do {             \
        OK(x);       \
        ++g_calls;   \
    } while (0)
#endif
// Three forms of a refusal.  A driver's REFUSED is the first of them, or the one it names before it includes this header
// (#define REFUSED REFUSED_MSG).
#ifndef REFUSED
#define REFUSED REFUSED_CODE
#endif
// counted: the code, and no launch (single-threaded part only)
#define REFUSED_CODE(x, code)                                              \
    do {                                                                   \
        const unsigned long long before_ = lr::g_stub_launches.load();     \
        CHECK((x) == (code));                                              \
        CHECK(lr::g_stub_launches.load() == before_);                      \
        ++g_refusals;                                                      \
    } while (0)
// logged: the code as CHECK sees it, and the message its caller reads goes to the log that driver_end prints (tests/cpp/expected/)
static std::vector<std::string> g_refusal_log;
#define REFUSED_MSG(cond)                                \
    do {                                                 \
        CHECK(cond);                                     \
        g_refusal_log.push_back(lr_last_error_string()); \
    } while (0)
// both: the code, no launch of any kind, and the message to the log
#define REFUSED_MSG_NO_LAUNCH(x, code)                                                                                                       \
    do {                                                                                                                                     \
        const unsigned long long a_ = lr::g_stub_launches.load(), b_ = lr::g_lincomb_launches.load(), c_ = lr::g_combine_launches.load();    \
        CHECK((x) == (code));                                                                                                                \
        CHECK(lr::g_stub_launches.load() == a_ && lr::g_lincomb_launches.load() == b_ && lr::g_combine_launches.load() == c_);               \
        g_refusal_log.push_back(lr_last_error_string());                                                                                     \
    } while (0)

// DefaultParams[PN15QP880]'s first primes (congruent to 1 modulo 2^16): Q5 and P3 as that set has them, M8 the two in one row ...
static const uint64_t Q5[5] = {1125899908022273ull, 1099512938497ull, 1099514314753ull, 1099515691009ull, 36028797019488257ull};
static const uint64_t P3[3] = {1125899908612097ull, 1125899909398529ull, 36028797023420417ull};
static const uint64_t M8[8] = {1125899908022273ull, 1099512938497ull,    1099514314753ull,    1099515691009ull,
                               36028797019488257ull, 1125899908612097ull, 1125899909398529ull, 36028797023420417ull};
// ... and Qm with a fifth 40-bit prime in place of the 55-bit one: Q from its front, P behind it
static const uint64_t Qm[5] = {1125899908022273ull, 1099512938497ull, 1099514314753ull, 1099515691009ull, 1099516280833ull};
// DefaultParams[PN16QP1761]'s first primes: congruent to 1 modulo 2^17 (N = 2^16)
static const uint64_t Q16[4] = {36028797019488257ull, 35184372744193ull, 35184373006337ull, 35184376545281ull};
static const uint64_t P16[2] = {36028797023420417ull, 36028797024206849ull};
// 64 primes congruent to 1 modulo 32 from 2^40 up: with one limb of P, one row more than Q||P may hold
static const uint64_t Q64[64] = {
    1099511627873ull, 1099511628161ull, 1099511628769ull, 1099511629121ull, 1099511629409ull, 1099511629537ull, 1099511629889ull, 1099511629921ull,
    1099511630177ull, 1099511630209ull, 1099511630561ull, 1099511630593ull, 1099511630849ull, 1099511631457ull, 1099511631937ull, 1099511632993ull,
    1099511633153ull, 1099511633377ull, 1099511634017ull, 1099511634113ull, 1099511635009ull, 1099511635361ull, 1099511636129ull, 1099511636161ull,
    1099511636833ull, 1099511637857ull, 1099511638177ull, 1099511638241ull, 1099511638529ull, 1099511638817ull, 1099511639297ull, 1099511639393ull,
    1099511639713ull, 1099511640001ull, 1099511641153ull, 1099511641729ull, 1099511641889ull, 1099511642209ull, 1099511642401ull, 1099511643137ull,
    1099511643521ull, 1099511643617ull, 1099511644321ull, 1099511646017ull, 1099511646241ull, 1099511646433ull, 1099511646529ull, 1099511646721ull,
    1099511647009ull, 1099511647841ull, 1099511647873ull, 1099511648513ull, 1099511649121ull, 1099511649409ull, 1099511649473ull, 1099511649793ull,
    1099511651009ull, 1099511651041ull, 1099511651137ull, 1099511651297ull, 1099511652257ull, 1099511652769ull, 1099511652929ull, 1099511653249ull};

static lr_poly *poly(lr_context *ctx, int limbs, int batch) {
    lr_poly *p = nullptr;
    OK(lr_poly_alloc(ctx, limbs, batch, &p));
    return p;
}

// contextQ over the first nq of `primes` and contextP over the np behind them (np = 0: no contextP), with `opt` or with the defaults
struct Rings {
    lr_context *q = nullptr, *p = nullptr;
    int nq, np;
    Rings(uint64_t N, const uint64_t *primes, int nq_, int np_, const lr_options *opt) : nq(nq_), np(np_) {
        OK(opt ? lr_context_create_ex(N, primes, nq, 0, opt, &q) : lr_context_create(N, primes, nq, 0, &q));
        if (np) OK(opt ? lr_context_create_ex(N, primes + nq, np, 0, opt, &p) : lr_context_create(N, primes + nq, np, 0, &p));
    }
    ~Rings() {
        if (p) OK(lr_context_destroy(p));
        OK(lr_context_destroy(q));
    }
};

// The tail of main.  `what` names the checks the driver asks for: ALLOCATIONS and EVENTS, that every pool, table, staging buffer or event
// went with its handle; LOG, that the refusal log holds one message per refusal of `refused`, and its print between the two marker lines.
// Then the summary line -- the driver's own text, and the failures -- and the exit code: 0 = every check held.
enum : unsigned { ALLOCATIONS = 1, EVENTS = 2, LOG = 4 };
static int driver_end(unsigned what, int refused, const char *summary, ...) {
    if (what & ALLOCATIONS) CHECK(hipstub_live_allocations() == 0);
    if (what & EVENTS) CHECK(hipstub_live_events() == 0);
    if (what & LOG) {
        CHECK((int)g_refusal_log.size() == refused);
        std::printf("refusal messages begin\n");
        for (const std::string &m : g_refusal_log) std::printf("%s\n", m.c_str());
        std::printf("refusal messages end\n");
    }
    va_list args;
    va_start(args, summary);
    std::vprintf(summary, args);
    va_end(args);
    std::printf(", failures %d\n", g_fail.load());
    return g_fail.load() ? 1 : 0;
}
