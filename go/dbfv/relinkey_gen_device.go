// Replacement bodies for github.com/ldsec/lattigo/dbfv (v1.3.1), relinkey_gen.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from relinkey_gen.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_setup.py.
//
// The patch to upstream dbfv/relinkey_gen.go, line numbers of v1.3.1:
//
//	delete  GenShareRoundOne         :215  -> below: beta noise polys in compact form, then ONE call, Setup.RkgRound1 (digit add and the
//	                                        product with u in one pass); crp crosses as one image, the share comes back member by member
//	delete  GenShareRoundTwo         :277  -> below: per digit e1 then e2 in compact form, Setup.RkgRound2
//	delete  GenShareRoundThree       :322  -> below: Setup.RkgRound3; u - sk stays in registers, tmpPoly1 / polypool unused
//	delete  AggregateShareRoundOne   :262  -> below: Setup.Aggregate over two images of beta polys
//	delete  AggregateShareRoundTwo   :307  -> below: the same over two pair images
//	delete  AggregateShareRoundThree :336  -> below
//	delete  GenRelinearizationKey    :343  -> below: Setup.RkgKey in place on the round-two image, downloaded into the key's evakey
//	keep    NewEkgProtocol, NewEphemeralKey, AllocateShares, the six marshalers and the struct
package dbfv

import (
	"sync"

	"github.com/ldsec/lattigo/bfv"
	"github.com/ldsec/lattigo/ring"
)

var deviceRKGProtocols sync.Map // *RKGProtocol -> *ring.Setup

func (ekg *RKGProtocol) dev() *ring.Setup {
	if s, ok := deviceRKGProtocols.Load(ekg); ok {
		return s.(*ring.Setup)
	}
	s := ring.NewSetup(ekg.context.contextQ, ekg.context.contextP, 1)
	actual, _ := deviceRKGProtocols.LoadOrStore(ekg, s)
	return actual.(*ring.Setup)
}

// ReleaseDevice drops the protocol's device state and its entry in deviceRKGProtocols.
func (ekg *RKGProtocol) ReleaseDevice() {
	deviceRKGProtocols.Delete(ekg)
}

// GenShareRoundOne (:215).
func (ekg *RKGProtocol) GenShareRoundOne(u, sk *ring.Poly, crp []*ring.Poly, shareOut RKGShareRoundOne) {
	beta := ekg.context.params.Beta()
	n := ekg.context.n
	noise := make([]byte, beta*n)
	for i := uint64(0); i < beta; i++ {
		ekg.context.gaussianSampler.SampleCompact(noise[i*n : (i+1)*n])
	}
	d := ekg.dev()
	out := d.NewImage(int(beta))
	d.RkgRound1(u, sk, d.ShareImage(crp), noise, []*ring.Poly{out})
	d.DownloadShare(out, shareOut)
}

// AggregateShareRoundOne (:262).
func (ekg *RKGProtocol) AggregateShareRoundOne(share1, share2, shareOut RKGShareRoundOne) {
	d := ekg.dev()
	out := d.NewImage(len(shareOut))
	d.Aggregate([]*ring.Poly{d.ShareImage(share1), d.ShareImage(share2)}, out)
	d.DownloadShare(out, shareOut)
}

// GenShareRoundTwo (:277).
func (ekg *RKGProtocol) GenShareRoundTwo(round1 RKGShareRoundOne, sk *ring.Poly, crp []*ring.Poly, shareOut RKGShareRoundTwo) {
	beta := 2 * ekg.context.params.Beta()
	n := ekg.context.n
	noise := make([]byte, beta*n)
	for i := uint64(0); i < beta; i++ {
		ekg.context.gaussianSampler.SampleCompact(noise[i*n : (i+1)*n])
	}
	d := ekg.dev()
	out := d.NewImage(int(beta))
	d.RkgRound2(d.ShareImage(round1), sk, d.ShareImage(crp), noise, []*ring.Poly{out})
	d.DownloadPairs(out, shareOut)
}

// AggregateShareRoundTwo (:307).
func (ekg *RKGProtocol) AggregateShareRoundTwo(share1, share2, shareOut RKGShareRoundTwo) {
	d := ekg.dev()
	out := d.NewImage(2 * len(shareOut))
	d.Aggregate([]*ring.Poly{d.PairImage(share1), d.PairImage(share2)}, out)
	d.DownloadPairs(out, shareOut)
}

// GenShareRoundThree (:322).
func (ekg *RKGProtocol) GenShareRoundThree(round2 RKGShareRoundTwo, u, sk *ring.Poly, shareOut RKGShareRoundThree) {
	beta := ekg.context.params.Beta()
	n := ekg.context.n
	noise := make([]byte, beta*n)
	for i := uint64(0); i < beta; i++ {
		ekg.context.gaussianSampler.SampleCompact(noise[i*n : (i+1)*n])
	}
	d := ekg.dev()
	out := d.NewImage(int(beta))
	d.RkgRound3(d.PairImage(round2), u, sk, noise, []*ring.Poly{out})
	d.DownloadShare(out, shareOut)
}

// AggregateShareRoundThree (:336).
func (ekg *RKGProtocol) AggregateShareRoundThree(share1, share2, shareOut RKGShareRoundThree) {
	d := ekg.dev()
	out := d.NewImage(len(shareOut))
	d.Aggregate([]*ring.Poly{d.ShareImage(share1), d.ShareImage(share2)}, out)
	d.DownloadShare(out, shareOut)
}

// GenRelinearizationKey (:343).
func (ekg *RKGProtocol) GenRelinearizationKey(round2 RKGShareRoundTwo, round3 RKGShareRoundThree, evalKeyOut *bfv.EvaluationKey) {
	d := ekg.dev()
	key := d.PairImage(round2)
	d.RkgKey(key, d.ShareImage(round3), key)
	d.DownloadPairs(key, evalKeyOut.Get()[0].Get())
}
