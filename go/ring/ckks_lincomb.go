package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"unsafe"
)

// CkksLinCombConsts is what the scalar lines of res = c0 + sum c_k ct_k yield (lr_ckks_lincomb_constants): the reference's chain of one
// AddConst and per term MultByConstAndAdd -- with the MultByConst calls on the receiver that equalise scales -- in the caller's order
// (ckks/polynomial_evaluation.go:142-159, ckks/evaluator.go:373-734).  Pre, Lo and Hi hold LevelAfter+1 words per term, one row after
// the other; AddLo / AddHi are nil without a constant term.
type CkksLinCombConsts struct {
	LevelAfter   uint64
	ScaleAfter   float64
	AddLo, AddHi []uint64
	HasPre       []uint8
	Pre, Lo, Hi  []uint64
}

// CkksLinCombTerm is one c_k ct_k as the scalar side sees it: the constant, and the ciphertext's scale and level.
type CkksLinCombTerm struct {
	Constant complex128
	Scale    float64
	Level    uint64
}

// CkksLinCombConstants runs the scalar side on the host: no context, no device.  nttPsi1[i] is GetNttPsi()[i][1]; c0 == nil: no
// AddConst.  Outside the domain in which Go's float-to-integer conversions are the same on every machine (lattigo_ring.h) it panics
// with the library's message.
func CkksLinCombConstants(moduli, nttPsi1 []uint64, defaultScale float64, resLevel uint64, resScale float64, c0 *complex128, terms []CkksLinCombTerm) *CkksLinCombConsts {
	if len(nttPsi1) != len(moduli) || len(moduli) == 0 {
		panic("cannot CkksLinCombConstants: one root word per modulus")
	}
	n, limbs := len(terms), len(moduli)
	re, im, sc := make([]C.double, n+1), make([]C.double, n+1), make([]C.double, n+1)
	lv := make([]C.int, n+1)
	for k, t := range terms {
		re[k], im[k], sc[k], lv[k] = C.double(real(t.Constant)), C.double(imag(t.Constant)), C.double(t.Scale), C.int(t.Level)
	}
	out := &CkksLinCombConsts{HasPre: make([]uint8, n+1), Pre: make([]uint64, n*limbs+1), Lo: make([]uint64, n*limbs+1), Hi: make([]uint64, n*limbs+1)}
	addLo, addHi := make([]uint64, limbs), make([]uint64, limbs)
	var hasConst C.int
	var c0re, c0im C.double
	if c0 != nil {
		hasConst, c0re, c0im = 1, C.double(real(*c0)), C.double(imag(*c0))
	}
	var levelAfter C.int
	var scaleAfter C.double
	u64 := func(s []uint64) *C.uint64_t { return (*C.uint64_t)(unsafe.Pointer(&s[0])) }
	call(func() C.int {
		return C.lr_ckks_lincomb_constants(u64(moduli), u64(nttPsi1), C.int(limbs), C.double(defaultScale), C.int(resLevel), C.double(resScale), hasConst, c0re, c0im, C.int(n), &re[0], &im[0], &sc[0], &lv[0], &levelAfter, &scaleAfter, u64(addLo), u64(addHi), (*C.uint8_t)(unsafe.Pointer(&out.HasPre[0])), u64(out.Pre), u64(out.Lo), u64(out.Hi))
	})
	l1 := int(levelAfter) + 1
	out.LevelAfter, out.ScaleAfter = uint64(levelAfter), float64(scaleAfter)
	out.HasPre, out.Pre, out.Lo, out.Hi = out.HasPre[:n], out.Pre[:n*l1], out.Lo[:n*l1], out.Hi[:n*l1]
	if c0 != nil {
		out.AddLo, out.AddHi = addLo[:l1], addHi[:l1]
	}
	return out
}

// CkksLinComb runs the element loops of the same chain on both components of degree-1 ciphertexts as one device call (lr_ckks_lincomb):
// per limb 0 .. consts.LevelAfter and coefficient, acc = accumulate ? out : 0, CRed(acc + add) on component 0 with a constant, then per
// term MRed(acc, pre) where HasPre and CRed(acc + MRed(x, lo|hi)) -- T + 1 row passes per component where Context.HalfScalarOp per term
// and component moves 3 T to 5 T.  terms[k] = {c0, c1} of ct_k; no term may be a receiver poly.
func (c *Context) CkksLinComb(terms [][2]*Poly, consts *CkksLinCombConsts, accumulate bool, out [2]*Poly) {
	n := len(terms)
	if len(consts.HasPre) != n {
		panic("cannot CkksLinComb: the constants are those of another term count")
	}
	raw := C.malloc(C.size_t(2*n+1) * C.size_t(unsafe.Sizeof(uintptr(0))))
	defer C.free(raw)
	arr := polyArray(raw, 2*n+1)
	for k, t := range terms {
		c.use(t[0], t[1])
		arr[k], arr[n+k] = t[0].d, t[1].d
	}
	var acc C.int
	if accumulate {
		acc = 1
		c.use(out[0], out[1])
	} else {
		c.want(out[0], out[1])
	}
	u64 := func(s []uint64) *C.uint64_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.uint64_t)(unsafe.Pointer(&s[0]))
	}
	var hasPre *C.uint8_t
	if n > 0 {
		hasPre = (*C.uint8_t)(unsafe.Pointer(&consts.HasPre[0]))
	}
	t0 := (**C.lr_poly)(raw)
	t1 := (**C.lr_poly)(unsafe.Pointer(uintptr(raw) + uintptr(n)*unsafe.Sizeof(uintptr(0))))
	call(func() C.int {
		return C.lr_ckks_lincomb(c.h, C.int(consts.LevelAfter), C.int(n), t0, t1, hasPre, u64(consts.Pre), u64(consts.Lo), u64(consts.Hi), u64(consts.AddLo), u64(consts.AddHi), acc, out[0].d, out[1].d)
	})
	done(out[0], out[1])
}
