// What the drivers of the two evaluators' and the key switch's host side share (key_switch_driver.cpp, bfv_chain_driver.cpp,
// bfv_relin_deg_driver.cpp, ckks_chain_driver.cpp, ckks_basis_driver.cpp, ckks_lincomb_driver.cpp, ckks_combine_driver.cpp): the check
// macros with their counters, the primes and the poly allocator.  TEST INFRASTRUCTURE.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "lattigo_ring.h"

namespace lr {
extern std::atomic<unsigned long long> g_stub_launches;
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
// a refusal: the code, and no launch (single-threaded part only; a driver that also keeps the message defines its own REFUSED first)
#ifndef REFUSED
#define REFUSED(x, code)                                                   \
    do {                                                                   \
        const unsigned long long before_ = lr::g_stub_launches.load();     \
        CHECK((x) == (code));                                              \
        CHECK(lr::g_stub_launches.load() == before_);                      \
        ++g_refusals;                                                      \
    } while (0)
#endif

// DefaultParams[PN15QP880]'s first primes (congruent to 1 modulo 2^16)
static const uint64_t Q5[5] = {1125899908022273ull, 1099512938497ull, 1099514314753ull, 1099515691009ull, 36028797019488257ull};
static const uint64_t P3[3] = {1125899908612097ull, 1125899909398529ull, 36028797023420417ull};

static lr_poly *poly(lr_context *ctx, int limbs, int batch) {
    lr_poly *p = nullptr;
    OK(lr_poly_alloc(ctx, limbs, batch, &p));
    return p;
}
