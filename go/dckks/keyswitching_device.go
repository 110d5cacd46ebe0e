// Replacement bodies for github.com/ldsec/lattigo/dckks (v1.3.1), keyswitching.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from keyswitching.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_collective.py.
//
// The patch to upstream dckks/keyswitching.go, line numbers of v1.3.1:
//
//	delete  GenShare         :62-67    -> below: the smudging noise in compact form (KYSampler.SampleCompact), then ONE call,
//	                                      Collective.CkksCksShare at ct.Level(); the Sub into tmpDelta runs inside it
//	delete  genShareDelta    :69-94    -> below: the same call with skDelta as the input key and cks.tmp -- all zeros between calls, upstream
//	                                      zeroes it at :93 and nothing below writes it -- as the output key: CRed((x + q) - 0) = x
//	delete  AggregateShares  :99-101   -> below: Collective.Aggregate over the two shares
//	delete  KeySwitch        :104-108  -> below: Collective.Aggregate with ct[0] as the base (the Add), then with one share (the Copy)
//	keep    NewCKSProtocol :28-49, AllocateShare :52-54 and the struct: tmpDelta and hP stay allocated and unused
package dckks

import (
	"sync"

	"github.com/ldsec/lattigo/ckks"
	"github.com/ldsec/lattigo/ring"
)

var deviceCKSProtocols sync.Map // *CKSProtocol -> *ring.Collective

func (cks *CKSProtocol) dev() *ring.Collective {
	if c, ok := deviceCKSProtocols.Load(cks); ok {
		return c.(*ring.Collective)
	}
	c := ring.NewCollective(cks.dckksContext.contextQ, cks.dckksContext.contextP, 1)
	actual, _ := deviceCKSProtocols.LoadOrStore(cks, c)
	return actual.(*ring.Collective)
}

// ReleaseDevice drops the protocol's device state and its entry in deviceCKSProtocols.
func (cks *CKSProtocol) ReleaseDevice() {
	deviceCKSProtocols.Delete(cks)
}

// GenShare (:62).
func (cks *CKSProtocol) GenShare(skInput, skOutput *ring.Poly, ct *ckks.Ciphertext, shareOut CKSShare) {
	noise := make([]byte, cks.dckksContext.n)
	cks.gaussianSamplerSmudge.SampleCompact(noise)
	cks.dev().CkksCksShare(ct.Level(), skInput, skOutput, ct.Value()[1], noise, shareOut)
}

// genShareDelta (:69).
func (cks *CKSProtocol) genShareDelta(skDelta *ring.Poly, ct *ckks.Ciphertext, shareOut CKSShare) {
	noise := make([]byte, cks.dckksContext.n)
	cks.gaussianSamplerSmudge.SampleCompact(noise)
	cks.dev().CkksCksShare(ct.Level(), skDelta, cks.tmp, ct.Value()[1], noise, shareOut)
}

// AggregateShares (:99).
func (cks *CKSProtocol) AggregateShares(share1, share2, shareOut CKSShare) {
	cks.dev().Aggregate(uint64(len(share1.Coeffs)-1), nil, []*ring.Poly{share1, share2}, shareOut)
}

// KeySwitch (:104).
func (cks *CKSProtocol) KeySwitch(combined CKSShare, ct *ckks.Ciphertext, ctOut *ckks.Ciphertext) {
	ctOut.SetScale(ct.Scale())
	cks.dev().Aggregate(ct.Level(), ct.Value()[0], []*ring.Poly{combined}, ctOut.Value()[0])
	cks.dev().Aggregate(ct.Level(), nil, []*ring.Poly{ct.Value()[1]}, ctOut.Value()[1])
}
