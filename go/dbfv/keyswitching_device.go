// Replacement bodies for github.com/ldsec/lattigo/dbfv (v1.3.1), keyswitching.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from keyswitching.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_collective.py.
//
// The patch to upstream dbfv/keyswitching.go, line numbers of v1.3.1:
//
//	delete  GenShare         :74-79    -> below: the smudging noise in compact form (KYSampler.SampleCompact), then ONE call,
//	                                      Collective.BfvCksShare; the Sub into tmpDelta runs inside it
//	delete  genShareDelta    :81-109   -> below: the same call with skDelta as the input key and cks.tmpNtt -- all zeros between calls, upstream
//	                                      zeroes it at :107 and nothing below writes it -- as the output key: CRed((x + q) - 0) = x
//	delete  AggregateShares  :114-116  -> below: Collective.Aggregate over the two shares
//	delete  KeySwitch        :119-122  -> below: Collective.Aggregate with ct[0] as the base (the Add), then with one share (the Copy)
//	keep    NewCKSProtocol :38-59, AllocateShare :62-66, CKSShare.UnmarshalBinary :28-33 and the struct: tmpDelta and hP stay allocated
//	        and unused
package dbfv

import (
	"sync"

	"github.com/ldsec/lattigo/bfv"
	"github.com/ldsec/lattigo/ring"
)

var deviceCKSProtocols sync.Map // *CKSProtocol -> *ring.Collective

func (cks *CKSProtocol) dev() *ring.Collective {
	if c, ok := deviceCKSProtocols.Load(cks); ok {
		return c.(*ring.Collective)
	}
	c := ring.NewCollective(cks.context.contextQ, cks.context.contextP, 1)
	actual, _ := deviceCKSProtocols.LoadOrStore(cks, c)
	return actual.(*ring.Collective)
}

// ReleaseDevice drops the protocol's device state and its entry in deviceCKSProtocols.
func (cks *CKSProtocol) ReleaseDevice() {
	deviceCKSProtocols.Delete(cks)
}

// top is the level every BFV poly lives at.
func (cks *CKSProtocol) top() uint64 {
	return uint64(len(cks.context.contextQ.Modulus) - 1)
}

// GenShare (:74).
func (cks *CKSProtocol) GenShare(skInput, skOutput *ring.Poly, ct *bfv.Ciphertext, shareOut CKSShare) {
	noise := make([]byte, cks.context.n)
	cks.gaussianSamplerSmudge.SampleCompact(noise)
	cks.dev().BfvCksShare(skInput, skOutput, ct.Value()[1], noise, shareOut.Poly)
}

// genShareDelta (:81).
func (cks *CKSProtocol) genShareDelta(skDelta *ring.Poly, ct *bfv.Ciphertext, shareOut CKSShare) {
	noise := make([]byte, cks.context.n)
	cks.gaussianSamplerSmudge.SampleCompact(noise)
	cks.dev().BfvCksShare(skDelta, cks.tmpNtt, ct.Value()[1], noise, shareOut.Poly)
}

// AggregateShares (:114).
func (cks *CKSProtocol) AggregateShares(share1, share2, shareOut CKSShare) {
	cks.dev().Aggregate(cks.top(), nil, []*ring.Poly{share1.Poly, share2.Poly}, shareOut.Poly)
}

// KeySwitch (:119).
func (cks *CKSProtocol) KeySwitch(combined CKSShare, ct *bfv.Ciphertext, ctOut *bfv.Ciphertext) {
	cks.dev().Aggregate(cks.top(), ct.Value()[0], []*ring.Poly{combined.Poly}, ctOut.Value()[0])
	cks.dev().Aggregate(cks.top(), nil, []*ring.Poly{ct.Value()[1]}, ctOut.Value()[1])
}
