package ring

// #include "lattigo_ring.h"
import "C"

import (
	"runtime"
	"unsafe"
)

// CkksEncoder: what ckks.NewEncoder builds (ckks/encoder.go:31-69) -- rotGroup and the root table -- plus the decoder's CRT tables and
// its pool, with Encode / Decode (:78-168) on the device, bit for bit the reference.  roots is the reference's table roots[0 .. m],
// m = 2 N, as NewEncoder computed it with Go's math.Cos / math.Sin: those differ from the C library's in the last place, so the table
// crosses the boundary instead of being recomputed (nil: the library fills it with its libm).  A Go Poly is one polynomial, so the
// slice forms encode and decode one plaintext per call; EncodeDevice / DecodeDevice take the slots in device memory.
// contextQ is held so that the context outlives the handle that reads it.
type CkksEncoder struct {
	contextQ *Context
	MaxBatch int
	h        *C.lr_ckks_encoder
}

// NewCkksEncoder panics on a maxBatch outside 1 .. 65535, on a Q of more than 2048 bits and on a table that is not m + 1 long.
func NewCkksEncoder(contextQ *Context, maxBatch int, roots []complex128) *CkksEncoder {
	e := &CkksEncoder{contextQ: contextQ, MaxBatch: maxBatch}
	var table *C.double
	if roots != nil {
		if uint64(len(roots)) != 2*contextQ.N+1 {
			panic("cannot NewCkksEncoder: the root table must hold 2N + 1 entries")
		}
		table = (*C.double)(unsafe.Pointer(&roots[0]))
	}
	if DefaultOptions == nil {
		call(func() C.int { return C.lr_ckks_encoder_create(contextQ.h, C.int(maxBatch), table, &e.h) })
	} else {
		call(func() C.int {
			return C.lr_ckks_encoder_create_ex(contextQ.h, C.int(maxBatch), table, DefaultOptions.ptr(), &e.h)
		})
	}
	runtime.SetFinalizer(e, func(e *CkksEncoder) { C.lr_ckks_encoder_destroy(e.h) })
	return e
}

// Tables returns rotGroup (m / 2 entries, ckks/encoder.go:39-45) and the root table (m + 1 entries) as the handle holds them.
func (e *CkksEncoder) Tables() (rotGroup []uint64, roots []complex128) {
	rotGroup = make([]uint64, e.contextQ.N)
	roots = make([]complex128, 2*e.contextQ.N+1)
	rg, rt := (*C.uint64_t)(unsafe.Pointer(&rotGroup[0])), (*C.double)(unsafe.Pointer(&roots[0]))
	call(func() C.int { return C.lr_ckks_encoder_tables(e.h, rg, rt) })
	return
}

// Fused reports the route a call with this slot count takes: the fused kernels, or streaming stages around LDS tiles.
func (e *CkksEncoder) Fused(slots uint64) bool {
	var f C.int
	call(func() C.int { return C.lr_ckks_encoder_route(e.h, C.int(slots), &f) })
	return f != 0
}

// Encode (ckks/encoder.go:78): len(values) == slots, a power of two in 1 .. N/2; pt receives limbs 0 .. level in the NTT domain.
func (e *CkksEncoder) Encode(pt *Poly, values []complex128, slots uint64, level uint64, scale float64) {
	if uint64(len(values)) != slots || slots == 0 {
		panic("cannot Encode: number of values must be equal to slots")
	}
	src := (*C.double)(unsafe.Pointer(&values[0]))
	e.contextQ.want(pt)
	call(func() C.int { return C.lr_ckks_encode(e.h, src, C.int(slots), C.int(level), C.double(scale), 1, pt.d) })
	done(pt)
}

// Decode (ckks/encoder.go:119).
func (e *CkksEncoder) Decode(pt *Poly, slots uint64, level uint64, scale float64) []complex128 {
	if slots == 0 {
		panic("cannot Decode: slots must be a power of two between 1 and N/2")
	}
	res := make([]complex128, slots)
	dst := (*C.double)(unsafe.Pointer(&res[0]))
	e.contextQ.use(pt)
	call(func() C.int { return C.lr_ckks_decode(e.h, pt.d, C.int(slots), C.int(level), C.double(scale), 1, dst) })
	return res
}

// EncodeDevice / DecodeDevice: the slots of one plaintext in device memory (slots complex128 values), stream-ordered on contextQ's
// stream, no host copy; pt must be resident (Poly.Pin).
func (e *CkksEncoder) EncodeDevice(pt *Poly, values unsafe.Pointer, slots uint64, level uint64, scale float64) {
	e.contextQ.want(pt)
	call(func() C.int { return C.lr_ckks_encode_device(e.h, values, C.int(slots), C.int(level), C.double(scale), 1, pt.d) })
}

func (e *CkksEncoder) DecodeDevice(pt *Poly, slots uint64, level uint64, scale float64, values unsafe.Pointer) {
	e.contextQ.use(pt)
	call(func() C.int { return C.lr_ckks_decode_device(e.h, pt.d, C.int(slots), C.int(level), C.double(scale), 1, values) })
}
