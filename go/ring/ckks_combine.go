package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"unsafe"
)

// The ring operation of ckks evaluator.Add / AddNoMod / Sub / SubNoMod, as CkksCombineConstants and Context.CkksCombine take it.
const (
	CkksCombineAdd      = int(C.LR_ADD)
	CkksCombineAddNoMod = int(C.LR_ADD_NOMOD)
	CkksCombineSub      = int(C.LR_SUB)
	CkksCombineSubNoMod = int(C.LR_SUB_NOMOD)
)

// Which operand the receiver of evaluateInPlace is (ckks/evaluator.go:243, :270, :296).
const (
	CkksCombineOutNew  = int(C.LR_COMBINE_OUT_NEW)
	CkksCombineOutA    = int(C.LR_COMBINE_OUT_A)
	CkksCombineOutB    = int(C.LR_COMBINE_OUT_B)
	CkksCombineOutBoth = int(C.LR_COMBINE_OUT_BOTH)
)

// CkksCombineOperand is a ciphertext as the scalar side sees it.
type CkksCombineOperand struct {
	Degree, Level uint64
	Scale         float64
}

// CkksCombineConsts is what the scalar lines of evaluateInPlace yield (lr_ckks_combine_constants; ckks/evaluator.go:227-342 with the
// degree rules of Add / AddNoMod / Sub / SubNoMod): the result's level, scale and degree, which operand MultByConst multiplies (0 none,
// 1 a, 2 b: the one of the smaller scale) and by which Montgomery-form word per limb (nil when MultSide == 0).
type CkksCombineConsts struct {
	LevelAfter  uint64
	ScaleAfter  float64
	DegreeAfter uint64
	MultSide    int
	Mult        []uint64
}

// CkksCombineConstants runs the scalar side on the host: no context, no device.  Where the reference panics (both operands of degree 0,
// a receiver of too small a degree, a receiver above level 0 and below both operands, a degree-2 operand to be multiplied into the
// degree-1 pool ciphertext) and outside the domain of Go's float-to-integer conversions (lattigo_ring.h) it panics with the library's
// message.
func CkksCombineConstants(moduli []uint64, op int, a, b, out CkksCombineOperand, receiver int) *CkksCombineConsts {
	if len(moduli) == 0 {
		panic("cannot CkksCombineConstants: no modulus")
	}
	mult := make([]uint64, len(moduli))
	var levelAfter, degreeAfter, multSide C.int
	var scaleAfter C.double
	call(func() C.int {
		return C.lr_ckks_combine_constants((*C.uint64_t)(unsafe.Pointer(&moduli[0])), C.int(len(moduli)), C.int(op), C.int(a.Degree), C.int(a.Level), C.double(a.Scale), C.int(b.Degree), C.int(b.Level), C.double(b.Scale), C.int(out.Degree), C.int(out.Level), C.double(out.Scale), C.int(receiver), &levelAfter, &scaleAfter, &degreeAfter, &multSide, (*C.uint64_t)(unsafe.Pointer(&mult[0])))
	})
	res := &CkksCombineConsts{LevelAfter: uint64(levelAfter), ScaleAfter: float64(scaleAfter), DegreeAfter: uint64(degreeAfter), MultSide: int(multSide)}
	if res.MultSide != 0 {
		res.Mult = mult[:int(levelAfter)+1]
	}
	return res
}

// CkksCombineWords are the two half-vector words per limb of a multiplier or of AddConst's constant: Lo for the coefficients below
// N/2, Hi for the rest (a real constant: the same slice twice).
type CkksCombineWords struct {
	Lo, Hi []uint64
}

// CkksCombine runs the element loops of evaluateInPlace, with Sub's NegLvl tail, as one device call (lr_ckks_combine): per limb
// 0 .. level, coefficient and component, x = a_u (doubled first with doubleA, then MRed by ma), y = b_u (MRed by mb), the operation
// where both are present, the copy of a surplus component (negated when it comes from the subtrahend), and CRed(r + add) on component
// 0.  b == nil: no b.  out[u] may be a[u] or b[u] (upstream's in-place case); len(out) >= max(len(a), len(b)).  ma, mb, add == nil:
// that step does not run.
func (c *Context) CkksCombine(op int, level uint64, a, b, out []*Poly, doubleA bool, ma, mb, add *CkksCombineWords) {
	comps := len(a)
	if len(b) > comps {
		comps = len(b)
	}
	if len(a) == 0 || len(out) < comps {
		panic("cannot CkksCombine: no operand, or fewer receiver components than the larger operand has")
	}
	n := len(a) + len(b) + comps
	raw := C.malloc(C.size_t(n+1) * C.size_t(unsafe.Sizeof(uintptr(0))))
	defer C.free(raw)
	arr := polyArray(raw, n+1)
	c.use(a...)
	c.use(b...)
	isOperand := func(p *Poly) bool {
		for _, q := range a {
			if q == p {
				return true
			}
		}
		for _, q := range b {
			if q == p {
				return true
			}
		}
		return false
	}
	for u := 0; u < comps; u++ {
		if !isOperand(out[u]) {
			c.want(out[u])
		}
	}
	for u, p := range a {
		arr[u] = p.d
	}
	for u, p := range b {
		arr[len(a)+u] = p.d
	}
	for u := 0; u < comps; u++ {
		arr[len(a)+len(b)+u] = out[u].d
	}
	at := func(k int) **C.lr_poly {
		return (**C.lr_poly)(unsafe.Pointer(uintptr(raw) + uintptr(k)*unsafe.Sizeof(uintptr(0))))
	}
	var pb **C.lr_poly
	if len(b) > 0 {
		pb = at(len(a))
	}
	u64 := func(s []uint64) *C.uint64_t {
		if len(s) == 0 {
			return nil
		}
		return (*C.uint64_t)(unsafe.Pointer(&s[0]))
	}
	words := func(w *CkksCombineWords) (*C.uint64_t, *C.uint64_t) {
		if w == nil {
			return nil, nil
		}
		if uint64(len(w.Lo)) < level+1 || uint64(len(w.Hi)) < level+1 {
			panic("cannot CkksCombine: need level+1 words in each half")
		}
		return u64(w.Lo), u64(w.Hi)
	}
	maLo, maHi := words(ma)
	mbLo, mbHi := words(mb)
	addLo, addHi := words(add)
	var dbl C.int
	if doubleA {
		dbl = 1
	}
	call(func() C.int {
		return C.lr_ckks_combine(c.h, C.int(op), C.int(level), C.int(len(a)-1), at(0), C.int(len(b)-1), pb, dbl, maLo, maHi, mbLo, mbHi, addLo, addHi, at(len(a)+len(b)))
	})
	done(out[:comps]...)
}
