package ring

// #include "lattigo_ring.h"
import "C"

import (
	"runtime"
	"unsafe"
)

// BfvEncoder: what bfv.NewEncoder builds (bfv/encoder.go:28-68) -- contextT = (N, [t]), indexMatrix, deltaMont, the SimpleScaler and the
// one-limb pool -- with EncodeUint / EncodeInt / DecodeUint / DecodeInt (:70-182) on the device.  A Go Poly is one polynomial, so the
// slice forms encode and decode one plaintext per call; EncodeDevice / DecodeDevice take maxBatch plaintexts' slots in device memory.
// contextQ is held so that the context outlives the handle that reads it.
type BfvEncoder struct {
	contextQ *Context
	T        uint64
	MaxBatch int
	h        *C.lr_bfv_encoder
}

// NewBfvEncoder panics where bfv.NewEncoder's newBFVContext does: a t that does not allow an NTT at N.
func NewBfvEncoder(contextQ *Context, t uint64, maxBatch int) *BfvEncoder {
	e := &BfvEncoder{contextQ: contextQ, T: t, MaxBatch: maxBatch}
	if DefaultOptions == nil {
		call(func() C.int { return C.lr_bfv_encoder_create(contextQ.h, C.uint64_t(t), C.int(maxBatch), &e.h) })
	} else {
		call(func() C.int {
			return C.lr_bfv_encoder_create_ex(contextQ.h, C.uint64_t(t), C.int(maxBatch), DefaultOptions.ptr(), &e.h)
		})
	}
	runtime.SetFinalizer(e, func(e *BfvEncoder) { C.lr_bfv_encoder_destroy(e.h) })
	return e
}

// Tables returns indexMatrix (bfv/encoder.go:36-58) and deltaMont (GenLiftParams, bfv/utils.go:9-23) as the handle computed them.
func (e *BfvEncoder) Tables() (indexMatrix, deltaMont []uint64) {
	indexMatrix = make([]uint64, e.contextQ.N)
	deltaMont = make([]uint64, len(e.contextQ.Modulus))
	im, dm := (*C.uint64_t)(unsafe.Pointer(&indexMatrix[0])), (*C.uint64_t)(unsafe.Pointer(&deltaMont[0]))
	call(func() C.int { return C.lr_bfv_encoder_tables(e.h, im, dm) })
	return
}

// Fused reports the route the handle took at creation: the fused kernels, or the transform of contextT between small kernels.
func (e *BfvEncoder) Fused() bool {
	var f C.int
	call(func() C.int { return C.lr_bfv_encoder_route(e.h, &f) })
	return f != 0
}

// EncodeUint (bfv/encoder.go:71): the values are taken modulo t.
func (e *BfvEncoder) EncodeUint(coeffs []uint64, pt *Poly) {
	var src *C.uint64_t
	if len(coeffs) > 0 {
		src = (*C.uint64_t)(unsafe.Pointer(&coeffs[0]))
	}
	e.contextQ.want(pt)
	call(func() C.int { return C.lr_bfv_encode_uint(e.h, src, C.size_t(len(coeffs)), 1, pt.d) })
	done(pt)
}

// EncodeInt (bfv/encoder.go:95): a negative value goes to its residue in [0, t) (the reference's t + c for -t <= c < 0).
func (e *BfvEncoder) EncodeInt(coeffs []int64, pt *Poly) {
	var src *C.int64_t
	if len(coeffs) > 0 {
		src = (*C.int64_t)(unsafe.Pointer(&coeffs[0]))
	}
	e.contextQ.want(pt)
	call(func() C.int { return C.lr_bfv_encode_int(e.h, src, C.size_t(len(coeffs)), 1, pt.d) })
	done(pt)
}

// DecodeUint (bfv/encoder.go:140).
func (e *BfvEncoder) DecodeUint(pt *Poly) []uint64 {
	coeffs := make([]uint64, e.contextQ.N)
	dst := (*C.uint64_t)(unsafe.Pointer(&coeffs[0]))
	e.contextQ.use(pt)
	call(func() C.int { return C.lr_bfv_decode_uint(e.h, pt.d, 1, dst) })
	return coeffs
}

// DecodeInt (bfv/encoder.go:158): centred around zero.
func (e *BfvEncoder) DecodeInt(pt *Poly) []int64 {
	coeffs := make([]int64, e.contextQ.N)
	dst := (*C.int64_t)(unsafe.Pointer(&coeffs[0]))
	e.contextQ.use(pt)
	call(func() C.int { return C.lr_bfv_decode_int(e.h, pt.d, 1, dst) })
	return coeffs
}

// EncodeDevice / DecodeDevice: the slots of one plaintext in device memory (nValues / N words, uint64 or, signed, int64), stream-ordered
// on contextQ's stream, no host copy; pt must be resident (Poly.Pin).
func (e *BfvEncoder) EncodeDevice(values unsafe.Pointer, nValues int, signed bool, pt *Poly) {
	e.contextQ.want(pt)
	call(func() C.int { return C.lr_bfv_encode_device(e.h, values, C.size_t(nValues), 1, cBool(signed), pt.d) })
}

func (e *BfvEncoder) DecodeDevice(pt *Poly, signed bool, values unsafe.Pointer) {
	e.contextQ.use(pt)
	call(func() C.int { return C.lr_bfv_decode_device(e.h, pt.d, 1, cBool(signed), values) })
}

func cBool(b bool) C.int {
	if b {
		return 1
	}
	return 0
}
