// Replacement bodies for github.com/ldsec/lattigo/ckks (v1.3.1): the power basis of EvaluatePolyFast / Eco and EvaluateChebyFast / Eco,
// and PowerOf2.  This file is added to the package next to evaluator_device.go and combine_device.go (same rules: the module's ring
// package is replaced by go/ring of this repository, INTEGRATION.md section 3, and the upstream bodies of what is defined here are
// DELETED).  Same receivers, same signatures, so every upstream caller reaches the device call unchanged.
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image, INTEGRATION.md).
//
// The patch to upstream ckks/polynomial_evaluation.go, line numbers of v1.3.1:
//
//	delete  EvaluatePolyFast :10-30, EvaluatePolyEco :34-54 -> below: the two loops of computePowerBasis calls (:21-27, :45-51) become
//	                                      the list of their targets and ONE powerBasis call: ONE ring.CkksPowerBasisSchedule call
//	                                      (the recursion, MulRelinNew's level and scale and Rescale's loop for every product, host only)
//	                                      and ONE CkksPlan.PowerBasis call (the products of one depth as one MulRelin, their divisions and
//	                                      one pass that writes every C[n]).  recurse :111 and computePowerBasis :76 stay as they are
//	                                      (computePowerBasis has no caller left in the package)
//
// The patch to upstream ckks/chebyshev_evaluation.go:
//
//	delete  EvaluateChebyFast :10-32, EvaluateChebyEco :36-58 -> below: the head is combine_device.go's affineInPlace and Rescale, the
//	                                      two loops of computePowerBasisCheby calls (:23-29, :49-55) ONE powerBasis call.  recurseCheby
//	                                      :104 stays; computePowerBasisCheby keeps its replacement body in combine_device.go for callers
//	                                      that extend a basis one entry at a time
//
// The patch to upstream ckks/algorithms.go:
//
//	delete  PowerOf2 :9-31              -> below: op^(2^(logPow2-1)) is computePowerBasis(2^(logPow2-1)), ONE powerBasis call; the last
//	                                      squaring stays upstream's two lines into opOut (MulRelin, Rescale), which keep upstream's
//	                                      rules for a receiver that is the operand or lies at another level
//	keep    Power :42, PowerNew :34, InverseNew :76: upstream's bodies (they call MulRelin, Rescale and PowerOf2)
package ckks

import (
	"math/bits"

	"github.com/ldsec/lattigo/ring"
)

// powerBasis fills C with C[n] for every target, and what the recursion of computePowerBasis / computePowerBasisCheby creates on the
// way, from C[1]: the scalar lines on the host, the element loops as one device call.  C holds C[1] only, as in the four entry points.
func powerBasis(eval *evaluator, C map[uint64]*Ciphertext, targets []uint64, chebyshev bool, evakey *EvaluationKey) {
	context := eval.ckksContext.contextQ
	c1 := C[1]
	s := ring.CkksPowerBasisSchedule(context.Modulus, eval.ckksContext.scale, chebyshev, c1.Level(), c1.Scale(), targets)
	if len(s.Products) == 0 {
		return
	}
	outs := make([][2]*ring.Poly, len(s.Products))
	for k, p := range s.Products {
		ct := NewCiphertext(eval.params, 1, p.LevelAfter, p.ScaleAfter) // MulRelinNew :1005, then Rescale's DivScale and DropLevel
		eval.resident(ct.value[0], ct.value[1])
		outs[k] = [2]*ring.Poly{ct.value[0], ct.value[1]}
		C[p.N] = ct
	}
	eval.resident(c1.value[0], c1.value[1])
	eval.dev().plan.PowerBasis(c1.Level(), [2]*ring.Poly{c1.value[0], c1.value[1]}, s, eval.keyImage(evakey.evakey), outs)
}

// basisTargets is the n of the two loops of the four entry points: 2 .. 2^L, then 2^i for L < i < M.
func basisTargets(L, M uint64) (targets []uint64) {
	for i := uint64(2); i <= (1 << L); i++ {
		targets = append(targets, i)
	}
	for i := L + 1; i < M; i++ {
		targets = append(targets, 1<<i)
	}
	return
}

// EvaluatePolyFast (polynomial_evaluation.go:10).
func (eval *evaluator) EvaluatePolyFast(ct0 *Ciphertext, coeffs interface{}, evakey *EvaluationKey) (ctOut *Ciphertext) {
	degree, coeffsMap := convertCoeffs(coeffs)
	C := make(map[uint64]*Ciphertext)
	C[1] = ct0.CopyNew().Ciphertext()
	M := uint64(bits.Len64(degree - 1))
	L := uint64(M >> 1)
	powerBasis(eval, C, basisTargets(L, M), false, evakey)
	return recurse(degree, L, M, coeffsMap, C, eval, evakey)
}

// EvaluatePolyEco (polynomial_evaluation.go:34).
func (eval *evaluator) EvaluatePolyEco(ct0 *Ciphertext, coeffs interface{}, evakey *EvaluationKey) (ctOut *Ciphertext) {
	degree, coeffsMap := convertCoeffs(coeffs)
	C := make(map[uint64]*Ciphertext)
	C[1] = ct0.CopyNew().Ciphertext()
	M := uint64(bits.Len64(degree - 1))
	L := uint64(1)
	powerBasis(eval, C, basisTargets(L, M), false, evakey)
	return recurse(degree, L, M, coeffsMap, C, eval, evakey)
}

// EvaluateChebyFast (chebyshev_evaluation.go:10).
func (eval *evaluator) EvaluateChebyFast(op *Ciphertext, cheby *ChebyshevInterpolation, evakey *EvaluationKey) (opOut *Ciphertext) {
	C := make(map[uint64]*Ciphertext)
	C[1] = op.CopyNew().Ciphertext()
	eval.affineInPlace(C[1], 2/(cheby.b-cheby.a), (-cheby.a-cheby.b)/(cheby.b-cheby.a)) // :16-17
	eval.Rescale(C[1], eval.ckksContext.scale, C[1])
	M := uint64(bits.Len64(cheby.degree - 1))
	L := uint64(M >> 1)
	powerBasis(eval, C, basisTargets(L, M), true, evakey)
	return recurseCheby(cheby.degree, L, M, cheby.coeffs, C, eval, evakey)
}

// EvaluateChebyEco (chebyshev_evaluation.go:36).
func (eval *evaluator) EvaluateChebyEco(op *Ciphertext, cheby *ChebyshevInterpolation, evakey *EvaluationKey) (opOut *Ciphertext) {
	C := make(map[uint64]*Ciphertext)
	C[1] = op.CopyNew().Ciphertext()
	eval.affineInPlace(C[1], 2/(cheby.b-cheby.a), (-cheby.a-cheby.b)/(cheby.b-cheby.a)) // :42-43
	eval.Rescale(C[1], eval.ckksContext.scale, C[1])
	M := uint64(bits.Len64(cheby.degree - 1))
	L := uint64(1)
	powerBasis(eval, C, basisTargets(L, M), true, evakey)
	return recurseCheby(cheby.degree, L, M, cheby.coeffs, C, eval, evakey)
}

// PowerOf2 (algorithms.go:9): op^(2^logPow2).
func (eval *evaluator) PowerOf2(op *Ciphertext, logPow2 uint64, evakey *EvaluationKey, opOut *Ciphertext) {
	if logPow2 == 0 {
		if op != opOut {
			opOut.Copy(op.Element())
		}
		return
	}
	half := op
	if logPow2 > 1 {
		C := map[uint64]*Ciphertext{1: op}
		powerBasis(eval, C, []uint64{1 << (logPow2 - 1)}, false, evakey)
		half = C[1<<(logPow2-1)]
	}
	eval.MulRelin(half.Element(), half.Element(), evakey, opOut)
	eval.Rescale(opOut, eval.ckksContext.scale, opOut)
}
