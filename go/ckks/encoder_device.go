// Replacement bodies for github.com/ldsec/lattigo/ckks (v1.3.1), encoder.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from encoder.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_ckks_encoder.py.
//
// The patch to upstream ckks/encoder.go, line numbers of v1.3.1:
//
//	delete  Encode      :78-116   -> below: upstream's checks, then ONE call, CkksEncoder.Encode (invfft, the scatter with gap,
//	                                 scaleUpVecExact into limbs 0 .. Level() and NTTLvl)
//	delete  Decode      :119-168  -> below: ONE call, CkksEncoder.Decode (InvNTTLvl, the CRT and centring that PolyToBigint / Mod / Cmp / Sub
//	                                 did on big.Int, scaleDown, fft)
//	delete  invfftlazy  :170-193, invfft :195-202, fft :204-226  -> nothing calls them any more (their butterflies live inside the kernels)
//	keep    NewEncoder :31-69 (roots is passed to the device as it stands: Go's math.Cos / math.Sin differ from the C library's in the last
//	        place, and parity needs this table; values, valuesfloat, bigintCoeffs, qHalf, polypool and rotGroup are no longer read) and
//	        EncodeNew :71-75 (it calls Encode)
package ckks

import (
	"sync"

	"github.com/ldsec/lattigo/ring"
)

var deviceCkksEncoders sync.Map // *encoder -> *ring.CkksEncoder

func (encoder *encoder) dev() *ring.CkksEncoder {
	if e, ok := deviceCkksEncoders.Load(encoder); ok {
		return e.(*ring.CkksEncoder)
	}
	e := ring.NewCkksEncoder(encoder.ckksContext.contextQ, 1, encoder.roots)
	actual, _ := deviceCkksEncoders.LoadOrStore(encoder, e)
	return actual.(*ring.CkksEncoder)
}

// ReleaseDevice drops the encoder's device state and its entry in deviceCkksEncoders.
func (encoder *encoder) ReleaseDevice() {
	deviceCkksEncoders.Delete(encoder)
}

// Encode (:78).  Upstream's check at :84 (`slots == 0 && slots&(slots-1) == 0`) never rejects a slot count that is not a power of two;
// the device call does, with the message upstream meant.
func (encoder *encoder) Encode(plaintext *Plaintext, values []complex128, slots uint64) {
	if uint64(len(values)) > encoder.ckksContext.maxSlots || uint64(len(values)) > slots {
		panic("cannot Encode: too many values for the given number of slots")
	}
	if slots == 0 || slots&(slots-1) != 0 {
		panic("cannot Encode: slots must be a power of two between 1 and N/2")
	}
	if uint64(len(values)) != slots {
		panic("cannot Encode: number of values must be equal to slots")
	}
	encoder.dev().Encode(plaintext.value, values, slots, plaintext.Level(), plaintext.scale)
}

// Decode (:119).
func (encoder *encoder) Decode(plaintext *Plaintext, slots uint64) (res []complex128) {
	return encoder.dev().Decode(plaintext.value, slots, plaintext.Level(), plaintext.scale)
}
