// Replacement bodies for github.com/ldsec/lattigo/bfv (v1.3.1), encoder.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from encoder.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_bfv_encoder.py.
//
// The patch to upstream bfv/encoder.go, line numbers of v1.3.1:
//
//	delete  EncodeUint       :71-91    -> below: ONE call, BfvEncoder.EncodeUint (the scatter through indexMatrix, InvNTT over contextT
//	                                      and the lift by deltaMont into every limb of Q)
//	delete  EncodeInt        :95-119   -> below: ONE call, BfvEncoder.EncodeInt (a negative value as its residue modulo t: upstream's
//	                                      t + c for -t <= c < 0)
//	delete  encodePlaintext  :121-137  -> nothing calls it any more (its loops over Coeffs live inside the kernels)
//	delete  DecodeUint       :140-154  -> below: ONE call, BfvEncoder.DecodeUint (SimpleScaler.Scale, NTT over contextT, the gather)
//	delete  DecodeInt        :158-182  -> below: ONE call, BfvEncoder.DecodeInt (the same, centred around zero)
//	keep    NewEncoder :28-68 (indexMatrix feeds the length checks below; its simplescaler, polypool and deltaMont are no longer read)
package bfv

import (
	"sync"

	"github.com/ldsec/lattigo/ring"
)

var deviceEncoders sync.Map // *encoder -> *ring.BfvEncoder

func (encoder *encoder) dev() *ring.BfvEncoder {
	if e, ok := deviceEncoders.Load(encoder); ok {
		return e.(*ring.BfvEncoder)
	}
	e := ring.NewBfvEncoder(encoder.bfvContext.contextQ, encoder.params.T, 1)
	actual, _ := deviceEncoders.LoadOrStore(encoder, e)
	return actual.(*ring.BfvEncoder)
}

// ReleaseDevice drops the encoder's device state and its entry in deviceEncoders.
func (encoder *encoder) ReleaseDevice() {
	deviceEncoders.Delete(encoder)
}

// EncodeUint (:71).
func (encoder *encoder) EncodeUint(coeffs []uint64, plaintext *Plaintext) {
	if len(coeffs) > len(encoder.indexMatrix) {
		panic("cannot EncodeUint: invalid input to encode (number of coefficients must be smaller or equal to the context)")
	}
	if len(plaintext.value.Coeffs[0]) != len(encoder.indexMatrix) {
		panic("cannot EncodeUint: invalid plaintext to receive encoding (number of coefficients does not match the context of the encoder)")
	}
	encoder.dev().EncodeUint(coeffs, plaintext.value)
}

// EncodeInt (:95).
func (encoder *encoder) EncodeInt(coeffs []int64, plaintext *Plaintext) {
	if len(coeffs) > len(encoder.indexMatrix) {
		panic("cannot EncodeInt: invalid input to encode (number of coefficients must be smaller or equal to the context)")
	}
	if len(plaintext.value.Coeffs[0]) != len(encoder.indexMatrix) {
		panic("cannot EncodeInt: invalid plaintext to receive encoding (number of coefficients does not match the context of the encoder)")
	}
	encoder.dev().EncodeInt(coeffs, plaintext.value)
}

// DecodeUint (:140).
func (encoder *encoder) DecodeUint(plaintext *Plaintext) (coeffs []uint64) {
	return encoder.dev().DecodeUint(plaintext.value)
}

// DecodeInt (:158).
func (encoder *encoder) DecodeInt(plaintext *Plaintext) (coeffs []int64) {
	return encoder.dev().DecodeInt(plaintext.value)
}
