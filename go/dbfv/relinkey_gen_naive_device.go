// Replacement bodies for github.com/ldsec/lattigo/dbfv (v1.3.1), relinkey_gen_naive.go: this file is added to the package, the module's ring package
// is replaced by go/ring of this repository (INTEGRATION.md section 3), and the upstream bodies of the methods defined here are DELETED
// from relinkey_gen_naive.go (same receivers and signatures: Go has no virtual dispatch, see go/ckks/evaluator_device.go).
//
// NOT COMPILED IN THIS REPOSITORY'S PIPELINE (no Go toolchain in the image); statically checked by tests/test_go_setup.py.
//
// The patch to upstream dbfv/relinkey_gen_naive.go, line numbers of v1.3.1:
//
//	delete  GenShareRoundOne       :59  -> below: the noise of every digit (two polys each), then the ternaries, in upstream's order, in
//	                                        compact form; ONE call, Setup.RkgNaiveRound1(ring.SetupBFV)
//	delete  GenShareRoundTwo       :135  -> below: per digit the ternary v, then e2 and e3; Setup.RkgNaiveRound2
//	delete  AggregateShareRoundOne :117  -> below: Setup.Aggregate over two pair images
//	delete  AggregateShareRoundTwo :176  -> below
//	delete  GenRelinearizationKey  :187  -> below: Setup.RkgNaiveKey in place on the round-two image, downloaded into the key's evakey
//	keep    NewRKGProtocolNaive, AllocateShares, the four marshalers and the struct: polypool stays allocated and unused
package dbfv

import (
	"sync"

	"github.com/ldsec/lattigo/bfv"
	"github.com/ldsec/lattigo/ring"
)

var deviceRKGProtocolsNaive sync.Map // *RKGProtocolNaive -> *ring.Setup

func (rkg *RKGProtocolNaive) dev() *ring.Setup {
	if s, ok := deviceRKGProtocolsNaive.Load(rkg); ok {
		return s.(*ring.Setup)
	}
	s := ring.NewSetup(rkg.context.contextQ, rkg.context.contextP, 1)
	actual, _ := deviceRKGProtocolsNaive.LoadOrStore(rkg, s)
	return actual.(*ring.Setup)
}

// ReleaseDevice drops the protocol's device state and its entry in deviceRKGProtocolsNaive.
func (rkg *RKGProtocolNaive) ReleaseDevice() {
	deviceRKGProtocolsNaive.Delete(rkg)
}

// GenShareRoundOne (:59): upstream samples e0, e1 of every digit, then one ternary per digit.
func (rkg *RKGProtocolNaive) GenShareRoundOne(sk *ring.Poly, pk [2]*ring.Poly, shareOut RKGNaiveShareRoundOne) {
	beta, n := rkg.context.params.Beta(), rkg.context.n
	noise, coeffs, signs := make([]byte, 2*beta*n), make([]byte, beta*n>>3), make([]byte, beta*n>>3)
	for i := uint64(0); i < 2*beta; i++ {
		rkg.context.gaussianSampler.SampleCompact(noise[i*n : (i+1)*n])
	}
	for i := uint64(0); i < beta; i++ {
		ring.SampleTernaryBits(coeffs[i*n>>3:(i+1)*n>>3], signs[i*n>>3:(i+1)*n>>3])
	}
	d := rkg.dev()
	out := d.NewImage(int(2 * beta))
	d.RkgNaiveRound1(ring.SetupBFV, sk, pk, noise, coeffs, signs, []*ring.Poly{out})
	d.DownloadPairs(out, shareOut)
}

// AggregateShareRoundOne (:117).
func (rkg *RKGProtocolNaive) AggregateShareRoundOne(share1, share2, shareOut RKGNaiveShareRoundOne) {
	d := rkg.dev()
	out := d.NewImage(2 * len(shareOut))
	d.Aggregate([]*ring.Poly{d.PairImage(share1), d.PairImage(share2)}, out)
	d.DownloadPairs(out, shareOut)
}

// GenShareRoundTwo (:135): per digit upstream samples the ternary v, then e2, then e3.
func (rkg *RKGProtocolNaive) GenShareRoundTwo(round1 RKGNaiveShareRoundOne, sk *ring.Poly, pk [2]*ring.Poly, shareOut RKGNaiveShareRoundTwo) {
	beta, n := rkg.context.params.Beta(), rkg.context.n
	noise, coeffs, signs := make([]byte, 2*beta*n), make([]byte, beta*n>>3), make([]byte, beta*n>>3)
	for i := uint64(0); i < beta; i++ {
		ring.SampleTernaryBits(coeffs[i*n>>3:(i+1)*n>>3], signs[i*n>>3:(i+1)*n>>3])
		rkg.context.gaussianSampler.SampleCompact(noise[2*i*n : (2*i+1)*n])
		rkg.context.gaussianSampler.SampleCompact(noise[(2*i+1)*n : (2*i+2)*n])
	}
	d := rkg.dev()
	out := d.NewImage(int(2 * beta))
	d.RkgNaiveRound2(d.PairImage(round1), sk, pk, coeffs, signs, noise, []*ring.Poly{out})
	d.DownloadPairs(out, shareOut)
}

// AggregateShareRoundTwo (:176).
func (rkg *RKGProtocolNaive) AggregateShareRoundTwo(share1, share2, shareOut RKGNaiveShareRoundTwo) {
	d := rkg.dev()
	out := d.NewImage(2 * len(shareOut))
	d.Aggregate([]*ring.Poly{d.PairImage(share1), d.PairImage(share2)}, out)
	d.DownloadPairs(out, shareOut)
}

// GenRelinearizationKey (:187).
func (rkg *RKGProtocolNaive) GenRelinearizationKey(round2 RKGNaiveShareRoundTwo, evalKeyOut *bfv.EvaluationKey) {
	d := rkg.dev()
	key := d.PairImage(round2)
	d.RkgNaiveKey(key, key)
	d.DownloadPairs(key, evalKeyOut.Get()[0].Get())
}
