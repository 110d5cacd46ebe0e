// Replacement bodies for github.com/ldsec/lattigo/ckks (v1.3.1): evaluator.Add / AddNoMod / Sub / SubNoMod with evaluateInPlace, and the
// steps of the Chebyshev drivers that are not products.  This file is added to the package next to evaluator_device.go (same rules: the
// module's ring package is replaced by go/ring of this repository, INTEGRATION.md section 3, and the upstream bodies of what is defined
// here are DELETED).  Same receivers, same signatures for every method an upstream caller reaches, so recurse, recurseCheby, Power,
// the ...New wrappers and the examples reach the device call unchanged.
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image, INTEGRATION.md).
//
// The patch to upstream ckks/evaluator.go, line numbers of v1.3.1:
//
//	delete  evaluateInPlace :227-342   -> below, with the ring operation as a constant instead of a method value (its four callers
//	                                      are the four methods below): upstream's Resize and DropLevel on the receiver, then ONE
//	                                      ring.CkksCombineConstants call (which operand MultByConst multiplies, by which words, at
//	                                      which level; it panics where upstream panics) and ONE Context.CkksCombine call: MultByConst
//	                                      into the pool ciphertext or in place, the operation, CopyLvl of the surplus components and,
//	                                      for Sub / SubNoMod, their NegLvl -- 3 row passes per shared component where upstream's
//	                                      sequence moves 3 to 5, and no pool ciphertext
//	delete  Add             :154-157   -> below
//	delete  AddNoMod        :160-163   -> below
//	delete  Sub             :180-194   -> below: the NegLvl tail :186-192 is folded into the call
//	delete  SubNoMod        :197-211   -> below: the NegLvl tail :203-209 is folded into the call
//	keep    AddNew, AddNoModNew, SubNew, SubNoModNew (:166-225: they call the four above), Neg :345
//
// The patch to upstream ckks/chebyshev_evaluation.go:
//
//	delete  computePowerBasisCheby :60-101 -> below: the recursion, MulRelinNew and Rescale are upstream's; Add(C[n], C[n], C[n]) and
//	                                      then Sub(C[n], C[c], C[n]) or AddConst(C[n], -1, C[n]) (:92-99) become ONE Context.CkksCombine
//	                                      call with doubleA: 3 row passes per component where the two or three calls move up to 7
//	        EvaluateChebyFast :10-32, EvaluateChebyEco :36-58 are deleted whole and have their replacement bodies in
//	                                      power_basis_device.go (its patch list); there the two lines :16-17 / :42-43,
//	                                      `eval.MultByConst(C[1], 2/(cheby.b-cheby.a), C[1])` and
//	                                      `eval.AddConst(C[1], (-cheby.a-cheby.b)/(cheby.b-cheby.a), C[1])`, are the one line
//	                                      `eval.affineInPlace(C[1], 2/(cheby.b-cheby.a), (-cheby.a-cheby.b)/(cheby.b-cheby.a))`
//	                                      (defined below): both constants' words from ONE ring.CkksLinCombConstants call, the
//	                                      element loops as ONE Context.CkksCombine call
//	keep    recurseCheby :104 and, in polynomial_evaluation.go, recurse: they call MulRelin, Add, Rescale and
//	                                      evaluatePolyFromPowerBasis, each of which is a device call
package ckks

import (
	"math"

	"github.com/ldsec/lattigo/ring"
	"github.com/ldsec/lattigo/utils"
)

// Add (:154).
func (eval *evaluator) Add(op0, op1 Operand, ctOut *Ciphertext) {
	el0, el1, elOut := eval.getElemAndCheckBinary(op0, op1, ctOut, utils.MaxUint64(op0.Degree(), op1.Degree()))
	eval.evaluateInPlace(el0, el1, elOut, ring.CkksCombineAdd)
}

// AddNoMod (:160).
func (eval *evaluator) AddNoMod(op0, op1 Operand, ctOut *Ciphertext) {
	el0, el1, elOut := eval.getElemAndCheckBinary(op0, op1, ctOut, utils.MaxUint64(op0.Degree(), op1.Degree()))
	eval.evaluateInPlace(el0, el1, elOut, ring.CkksCombineAddNoMod)
}

// Sub (:180): the negation of the subtrahend's surplus components (:186-192) runs inside the call.
func (eval *evaluator) Sub(op0, op1 Operand, ctOut *Ciphertext) {
	el0, el1, elOut := eval.getElemAndCheckBinary(op0, op1, ctOut, utils.MaxUint64(op0.Degree(), op1.Degree()))
	eval.evaluateInPlace(el0, el1, elOut, ring.CkksCombineSub)
}

// SubNoMod (:197): as Sub (:203-209).
func (eval *evaluator) SubNoMod(op0, op1 Operand, ctOut *Ciphertext) {
	el0, el1, elOut := eval.getElemAndCheckBinary(op0, op1, ctOut, utils.MaxUint64(op0.Degree(), op1.Degree()))
	eval.evaluateInPlace(el0, el1, elOut, ring.CkksCombineSubNoMod)
}

// combineOperand is an element as the scalar side sees it.
func combineOperand(el *ckksElement) ring.CkksCombineOperand {
	return ring.CkksCombineOperand{Degree: el.Degree(), Level: el.Level(), Scale: el.Scale()}
}

// combineReceiver names which operand the receiver is (:243, :270, :296).
func combineReceiver(c0, c1, ctOut *ckksElement) int {
	switch {
	case ctOut == c0 && ctOut == c1:
		return ring.CkksCombineOutBoth
	case ctOut == c0:
		return ring.CkksCombineOutA
	case ctOut == c1:
		return ring.CkksCombineOutB
	}
	return ring.CkksCombineOutNew
}

// evaluateInPlace (:227): the scalar lines on the host, the element loops as one device call (patch list above).  The constants are
// taken BEFORE Resize and DropLevel touch the receiver, as upstream reads its levels and degrees at :231-234; a call that upstream
// would panic on panics here with the library's message, before anything is written.
func (eval *evaluator) evaluateInPlace(c0, c1, ctOut *ckksElement, op int) {
	context := eval.ckksContext.contextQ
	consts := ring.CkksCombineConstants(context.Modulus, op, combineOperand(c0), combineOperand(c1), combineOperand(ctOut), combineReceiver(c0, c1, ctOut))
	ctOut.Resize(eval.params, consts.DegreeAfter)                                                 // :237
	eval.DropLevel(ctOut.Ciphertext(), ctOut.Level()-utils.MinUint64(c0.Level(), c1.Level())) // :238 (a receiver at level 0 stays)
	var ma, mb *ring.CkksCombineWords
	switch consts.MultSide {
	case 1:
		ma = &ring.CkksCombineWords{Lo: consts.Mult, Hi: consts.Mult}
	case 2:
		mb = &ring.CkksCombineWords{Lo: consts.Mult, Hi: consts.Mult}
	}
	eval.resident(c0.value...)
	eval.resident(c1.value...)
	eval.resident(ctOut.value...)
	context.CkksCombine(op, consts.LevelAfter, c0.value, c1.value, ctOut.value, false, ma, mb, nil)
	ctOut.SetScale(consts.ScaleAfter) // :328 (and :259, :285 where the receiver is the multiplied operand)
}

// addConstWords are AddConst's per-limb words (:412-438) for `constant` on a ciphertext at `level` and `scale`.
func (eval *evaluator) addConstWords(constant complex128, level uint64, scale float64) *ring.CkksCombineWords {
	k := ring.CkksLinCombConstants(eval.ckksContext.contextQ.Modulus, eval.nttPsi1(), eval.ckksContext.scale, level, scale, &constant, nil)
	return &ring.CkksCombineWords{Lo: k.AddLo, Hi: k.AddHi}
}

func (eval *evaluator) nttPsi1() []uint64 {
	context := eval.ckksContext.contextQ
	psi1 := make([]uint64, len(context.Modulus))
	for i := range psi1 {
		psi1[i] = context.GetNttPsi()[i][1]
	}
	return psi1
}

// affineInPlace is MultByConst(ct, m, ct) followed by AddConst(ct, c, ct) (chebyshev_evaluation.go:16-17, :42-43) for float64 constants:
// the words of both from one host call, the element loops as one device call.  MultByConst scales a constant with a fractional part by
// the default scale (:656-667) and sets the ciphertext's scale (:733); AddConst then reads that scale (:420).
func (eval *evaluator) affineInPlace(ct *Ciphertext, m, c float64) {
	scale := float64(1)
	if m != 0 && m-float64(int64(m)) != 0 {
		scale = eval.ckksContext.scale
	}
	level := ct.Level()
	c0 := complex(c, 0)
	// a receiver already at ct.Scale() * scale takes the term without rescaling either side (:538, :546 do not fire): Lo / Hi are
	// MultByConst's words (:698-721), AddLo / AddHi AddConst's at the new scale
	k := ring.CkksLinCombConstants(eval.ckksContext.contextQ.Modulus, eval.nttPsi1(), eval.ckksContext.scale, level, ct.Scale()*scale, &c0,
		[]ring.CkksLinCombTerm{{Constant: complex(m, 0), Scale: ct.Scale(), Level: level}})
	eval.resident(ct.value...)
	eval.ckksContext.contextQ.CkksCombine(ring.CkksCombineAdd, level, ct.value, nil, ct.value, false,
		&ring.CkksCombineWords{Lo: k.Lo, Hi: k.Hi}, nil, &ring.CkksCombineWords{Lo: k.AddLo, Hi: k.AddHi})
	ct.SetScale(ct.Scale() * scale)
}

// computePowerBasisCheby (chebyshev_evaluation.go:60): C[n] = 2 C[a] C[b] - C[c]; after the product, one device call (patch list above).
func computePowerBasisCheby(n uint64, C map[uint64]*Ciphertext, evaluator *evaluator, evakey *EvaluationKey) {
	if C[n] == nil {
		a := uint64(math.Ceil(float64(n) / 2))
		b := n >> 1
		c := uint64(math.Abs(float64(a) - float64(b)))
		computePowerBasisCheby(a, C, evaluator, evakey)
		computePowerBasisCheby(b, C, evaluator, evakey)
		if c != 0 {
			computePowerBasisCheby(c, C, evaluator, evakey)
		}
		C[n] = evaluator.MulRelinNew(C[a], C[b], evakey)
		evaluator.Rescale(C[n], evaluator.ckksContext.scale, C[n])
		context := evaluator.ckksContext.contextQ
		cn := C[n]
		evaluator.resident(cn.value...)
		if c == 0 {
			// Add(C[n], C[n], C[n]) keeps level and scale (:92); AddConst(C[n], -1, C[n]) (:96) touches value[0] only
			add := evaluator.addConstWords(complex(-1, 0), cn.Level(), cn.Scale())
			context.CkksCombine(ring.CkksCombineAdd, cn.Level(), cn.value, nil, cn.value, true, nil, nil, add)
			return
		}
		// Sub(C[n], C[c], C[n]) (:98) after the doubling: the receiver is operand a
		cc := C[c]
		el0, el1, elOut := evaluator.getElemAndCheckBinary(cn, cc, cn, utils.MaxUint64(cn.Degree(), cc.Degree()))
		consts := ring.CkksCombineConstants(context.Modulus, ring.CkksCombineSub, combineOperand(el0), combineOperand(el1), combineOperand(elOut), ring.CkksCombineOutA)
		evaluator.DropLevel(cn, cn.Level()-utils.MinUint64(cn.Level(), cc.Level()))
		var ma, mb *ring.CkksCombineWords
		switch consts.MultSide {
		case 1:
			ma = &ring.CkksCombineWords{Lo: consts.Mult, Hi: consts.Mult}
		case 2:
			mb = &ring.CkksCombineWords{Lo: consts.Mult, Hi: consts.Mult}
		}
		evaluator.resident(cc.value...)
		context.CkksCombine(ring.CkksCombineSub, consts.LevelAfter, cn.value, cc.value, cn.value, true, ma, mb, nil)
		cn.SetScale(consts.ScaleAfter)
	}
}
