// What the launch stand-ins of this directory share (stub_launch.cpp, and one stub_<kernel file>.cpp per handle's kernel file), for the CPU
// build of the host side that the sanitizer tests run (tests/host_stub_build.py): the touches that stand for a kernel's reads and writes.
// A stand-in counts or records its launch and touches the first and the last byte of everything the real kernel would read or write, at
// the addresses the launch names.  "Device" memory is malloc'ed at its exact size, so a wrong size, stride, level or count in the host
// code is an AddressSanitizer report.  TEST INFRASTRUCTURE: no arithmetic of the hot path lives here.
#pragma once
#include "lr_arith.hpp"

namespace lr {

inline thread_local volatile u64 t_sink;          // (per thread: the reads are the point, not the sink)

// one word
inline void rd(const u64 *p) { t_sink = *p; }
// `count` elements from p on, read
template <class T>
inline void rd(const T *p, long long count) {
    if (count <= 0) return;
    t_sink = (u64)((const volatile unsigned char *)p)[0];
    t_sink = (u64)((const volatile unsigned char *)(p + count))[-1];
}
// `count` elements from p on, written (the values are kept): words as words, anything else by its first and last byte
inline void wr(u64 *p, long long count) {
    if (count <= 0) return;
    p[0] = p[0];
    p[count - 1] = p[count - 1];
}
template <class T>
inline void wr(T *p, long long count) {
    if (count <= 0) return;
    volatile unsigned char *b = (volatile unsigned char *)p, *e = (volatile unsigned char *)(p + count) - 1;
    *b = *b;
    *e = *e;
}

}  // namespace lr
