package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"unsafe"
)

// CkksBasisProduct is one product of a power basis as the scalar side yields it (lr_ckks_basis_product): C[N] = C[A] C[B] at MulLevel,
// NRescales iterations of Rescale's loop down to LevelAfter and ScaleAfter, and the Chebyshev tail -- 0 none, 1: 2 x - C[C] with
// MultSide as CkksCombineConstants names it, 2: 2 x - 1.
type CkksBasisProduct struct {
	N, A, B, C uint64
	MulLevel   uint64
	NRescales  uint64
	LevelAfter uint64
	Layer      int
	Tail       int
	MultSide   int
	ScaleAfter float64
}

// CkksBasisSchedule is what CkksPowerBasisSchedule yields: the products in the order the reference creates them and, per product, one
// row of len(moduli) words for the multiplier of tail 1 and one for the addend of tail 2 (zero where unused), as the library laid them out.
type CkksBasisSchedule struct {
	Products []CkksBasisProduct
	Mult     []uint64
	Add      []uint64
	RowWords int
	raw      []C.lr_ckks_basis_product
}

// Index returns the position of C[n] among the products, or -1.
func (s *CkksBasisSchedule) Index(n uint64) int {
	for k := range s.Products {
		if s.Products[k].N == n {
			return k
		}
	}
	return -1
}

// CkksPowerBasisSchedule runs the scalar lines of computePowerBasis (ckks/polynomial_evaluation.go:76-93) or, with chebyshev,
// computePowerBasisCheby (ckks/chebyshev_evaluation.go:60-101) for the targets in the caller's order, on the host: no context, no device
// (lr_ckks_power_basis_schedule).  Outside the domain the header states it panics with the library's message.
func CkksPowerBasisSchedule(moduli []uint64, defaultScale float64, chebyshev bool, c1Level uint64, c1Scale float64, targets []uint64) *CkksBasisSchedule {
	if len(moduli) == 0 {
		panic("cannot CkksPowerBasisSchedule: no modulus")
	}
	t32 := make([]C.uint32_t, len(targets)+1)
	for i, t := range targets {
		if t == 0 || t > 65535 {
			panic("cannot CkksPowerBasisSchedule: a target is 0 or above 65535")
		}
		t32[i] = C.uint32_t(t)
	}
	cheb := C.int(0)
	if chebyshev {
		cheb = 1
	}
	pm := (*C.uint64_t)(unsafe.Pointer(&moduli[0]))
	// the capacity protocol: the count first, then the buffers of that size
	count := C.int(-1)
	if rc, msg := status(func() C.int {
		return C.lr_ckks_power_basis_schedule(pm, C.int(len(moduli)), C.double(defaultScale), cheb, C.int(c1Level), C.double(c1Scale), C.int(len(targets)), &t32[0], 0, &count, nil, nil, nil)
	}); rc != C.LR_OK && count < 0 {
		panic("lattigo_ring: " + msg)
	}
	n := int(count)
	s := &CkksBasisSchedule{RowWords: len(moduli), raw: make([]C.lr_ckks_basis_product, n+1), Mult: make([]uint64, n*len(moduli)+1), Add: make([]uint64, n*len(moduli)+1)}
	call(func() C.int {
		return C.lr_ckks_power_basis_schedule(pm, C.int(len(moduli)), C.double(defaultScale), cheb, C.int(c1Level), C.double(c1Scale), C.int(len(targets)), &t32[0], C.int(n), &count, &s.raw[0], (*C.uint64_t)(unsafe.Pointer(&s.Mult[0])), (*C.uint64_t)(unsafe.Pointer(&s.Add[0])))
	})
	s.raw = s.raw[:n]
	s.Products = make([]CkksBasisProduct, n)
	for k, p := range s.raw {
		s.Products[k] = CkksBasisProduct{N: uint64(p.n), A: uint64(p.a), B: uint64(p.b), C: uint64(p.c), MulLevel: uint64(p.mul_level), NRescales: uint64(p.n_rescales), LevelAfter: uint64(p.level_after), Layer: int(p.layer), Tail: int(p.tail), MultSide: int(p.mult_side), ScaleAfter: float64(p.scale_after)}
	}
	return s
}

// PowerBasis runs the element loops of a schedule as ONE device call (lr_ckks_power_basis): c1 = C[1] at c1Level, outs[k] receives
// C[s.Products[k].N] on limbs 0 .. LevelAfter (it needs LevelAfter+1 limbs).  Bit for bit MulRelin, Rescale NRescales times and the
// CkksCombine call of the Chebyshev tail, per product.
func (p *CkksPlan) PowerBasis(c1Level uint64, c1 [2]*Poly, s *CkksBasisSchedule, evakey *Poly, outs [][2]*Poly) {
	n := len(s.Products)
	if len(outs) != n {
		panic("cannot PowerBasis: one output per product")
	}
	if n == 0 {
		return
	}
	p.contextQ.use(c1[0], c1[1])
	o0, o1 := make([]*Poly, n), make([]*Poly, n)
	for k := range outs {
		o0[k], o1[k] = outs[k][0], outs[k][1]
		p.contextQ.want(o0[k], o1[k])
	}
	t0, t1 := polyTable(o0), polyTable(o1)
	defer C.free(unsafe.Pointer(t0))
	defer C.free(unsafe.Pointer(t1))
	call(func() C.int {
		return C.lr_ckks_power_basis(p.h, C.int(n), &s.raw[0], (*C.uint64_t)(unsafe.Pointer(&s.Mult[0])), (*C.uint64_t)(unsafe.Pointer(&s.Add[0])), C.int(s.RowWords), C.int(c1Level), c1[0].d, c1[1].d, evakey.d, t0, t1)
	})
	done(o0...)
	done(o1...)
}
