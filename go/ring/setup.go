package ring

// #include <stdlib.h>
// #include "lattigo_ring.h"
import "C"

import (
	"runtime"
	"unsafe"
)

// Setup: what NewCKGProtocol, NewEkgProtocol, NewRKGProtocolNaive and NewRotKGProtocol of dckks and dbfv build -- polypool / tmpPoly over
// Q||P -- with CKGProtocol.GenShare, the rounds and GenRelinearizationKey of both RKG protocols, RTGProtocol.genShare and Finalize, and
// every Aggregate* on the device, after the sampling (lr_setup in include/lattigo_ring.h).  The randomness is the samplers' decisions in
// the compact form of BfvEncryptor, recorded by the same samplers (SampleTernaryBits, KYSampler.SampleCompact in bfv_encryptor.go): beta N
// bytes per share of beta polys cross to the device instead of beta polys over Q||P.
// A Go Poly is one polynomial; a share of beta polys (or of beta pairs) is an IMAGE: one device poly of batch beta (2 beta), made by
// NewImage, ShareImage or PairImage and read back by DownloadShare / DownloadPairs.  The pair image is the key image CkksPlan's key
// switch reads, so RkgKey, RkgNaiveKey and RtgKey leave a key where the evaluator finds it.  sk, u, crs and pk are plain polys over
// Q||P.  contextP nil is upstream's "P is empty": only CkgShare and Aggregate over single polys.
type Setup struct {
	contextQ, contextP *Context
	MaxBatch           int
	h                  *C.lr_setup
}

// The scheme whose lines RkgNaiveRound1 runs: dckks/relinkey_gen_naive.go:73-75 draws both noise polys into shareOut[i][0].
const (
	SetupBFV  = 0
	SetupCKKS = 1
)

func NewSetup(contextQ, contextP *Context, maxBatch int) *Setup {
	s := &Setup{contextQ: contextQ, contextP: contextP, MaxBatch: maxBatch}
	var hP *C.lr_context
	if contextP != nil {
		hP = contextP.h
	}
	if DefaultOptions == nil {
		call(func() C.int { return C.lr_setup_create(contextQ.h, hP, C.int(maxBatch), &s.h) })
	} else {
		call(func() C.int { return C.lr_setup_create_ex(contextQ.h, hP, C.int(maxBatch), DefaultOptions.ptr(), &s.h) })
	}
	runtime.SetFinalizer(s, func(s *Setup) { C.lr_setup_destroy(s.h) })
	return s
}

// Beta = params.Beta(): ceil(|Q| / |P|), the digits of a share.
func (s *Setup) Beta() int {
	if s.contextP == nil {
		panic("cannot Beta: modulus P is empty")
	}
	nQ, nP := len(s.contextQ.Modulus), len(s.contextP.Modulus)
	return (nQ + nP - 1) / nP
}

func (s *Setup) rows() int {
	if s.contextP == nil {
		return len(s.contextQ.Modulus)
	}
	return len(s.contextQ.Modulus) + len(s.contextP.Modulus)
}

// NewImage allocates a device poly of `members` polys over Q||P: the output of a share call or of a finalize step.
func (s *Setup) NewImage(members int) *Poly {
	img := &Poly{resident: true, dLimbs: s.rows()}
	call(func() C.int { return C.lr_poly_alloc(s.contextQ.h, C.int(s.rows()), C.int(members), &img.d) })
	runtime.SetFinalizer(img, func(q *Poly) { C.lr_poly_free(q.d) })
	return img
}

// ShareImage uploads a share of polys (RKGShareRoundOne, RKGShareRoundThree, RTGShare.Value, crp) as one image, member i = polys[i].
func (s *Setup) ShareImage(polys []*Poly) *Poly {
	img := s.NewImage(len(polys))
	for i, p := range polys {
		p.hostView()
		p.uploadTo(img.d, i)
	}
	return img
}

// PairImage uploads a share of pairs (RKGShareRoundTwo, both naive shares) as one image, member 2i = pairs[i][0], 2i+1 = pairs[i][1].
func (s *Setup) PairImage(pairs [][2]*Poly) *Poly {
	img := s.NewImage(2 * len(pairs))
	for i := range pairs {
		for k := 0; k < 2; k++ {
			pairs[i][k].hostView()
			pairs[i][k].uploadTo(img.d, 2*i+k)
		}
	}
	return img
}

func downloadMember(image *Poly, member int, dst *Poly) {
	for j := range dst.Coeffs {
		m, limb := C.int(member), C.int(j)
		p := (*C.uint64_t)(unsafe.Pointer(&dst.Coeffs[j][0]))
		call(func() C.int { return C.lr_poly_download_limb(image.d, m, limb, p) })
	}
	dst.hostWritten()
}

// DownloadShare copies the members of an image into a share of polys on the host (marshalling, the next party).
func (s *Setup) DownloadShare(image *Poly, polys []*Poly) {
	for i := range polys {
		downloadMember(image, i, polys[i])
	}
}

// DownloadPairs copies the members of an image into a share of pairs, or into SwitchingKey.evakey, on the host.
func (s *Setup) DownloadPairs(image *Poly, pairs [][2]*Poly) {
	for i := range pairs {
		downloadMember(image, 2*i, pairs[i][0])
		downloadMember(image, 2*i+1, pairs[i][1])
	}
}

// plain polys are bound and uploaded around a call as everywhere in this package; images (no Coeffs) live on the device
func (s *Setup) in(ps ...*Poly) {
	for _, p := range ps {
		if p.Coeffs != nil {
			s.contextQ.use(p)
		}
	}
}

func (s *Setup) out(ps ...*Poly) {
	for _, p := range ps {
		if p.Coeffs != nil {
			s.contextQ.want(p)
		}
	}
}

func finished(ps ...*Poly) {
	for _, p := range ps {
		if p.Coeffs != nil {
			done(p)
		}
	}
}

func (s *Setup) noiseLen(what string, polys int, noise []byte) {
	if len(noise) != polys*int(s.contextQ.N) {
		panic("cannot " + what + ": the compact randomness is N bytes per sampled poly")
	}
}

func (s *Setup) planeLen(what string, polys int, planes ...[]byte) {
	for _, b := range planes {
		if len(b) != polys*(int(s.contextQ.N)>>3) {
			panic("cannot " + what + ": the compact randomness is N/8 bytes per bit plane")
		}
	}
}

// CkgShare = CKGProtocol.GenShare (dbfv/publickey_gen.go:54-57): plain polys, noise N bytes.
func (s *Setup) CkgShare(sk, crs *Poly, noise []byte, shareOut *Poly) {
	s.noiseLen("CkgShare", 1, noise)
	s.in(sk, crs)
	s.out(shareOut)
	call(func() C.int { return C.lr_setup_ckg_share(s.h, sk.d, crs.d, bytePtr(noise), 1, shareOut.d) })
	finished(shareOut)
}

// RkgRound1 = GenShareRoundOne (dbfv/relinkey_gen.go:215-259) for len(shares) parties: crp and the shares are images of beta polys.
func (s *Setup) RkgRound1(u, sk, crp *Poly, noise []byte, shares []*Poly) {
	s.noiseLen("RkgRound1", len(shares)*s.Beta(), noise)
	s.in(u, sk)
	call(func() C.int { return C.lr_setup_rkg_round1(s.h, u.d, sk.d, crp.d, bytePtr(noise), C.int(len(shares)), keyHandles(shares)) })
}

// RkgRound2 = GenShareRoundTwo (:277-299): round1 = the aggregate image, the shares are pair images; per digit e1 before e2.
func (s *Setup) RkgRound2(round1, sk, crp *Poly, noise []byte, shares []*Poly) {
	s.noiseLen("RkgRound2", 2*len(shares)*s.Beta(), noise)
	s.in(sk)
	call(func() C.int { return C.lr_setup_rkg_round2(s.h, round1.d, sk.d, crp.d, bytePtr(noise), C.int(len(shares)), keyHandles(shares)) })
}

// RkgRound3 = GenShareRoundThree (:322-333): round2 = the aggregate pair image.
func (s *Setup) RkgRound3(round2, u, sk *Poly, noise []byte, shares []*Poly) {
	s.noiseLen("RkgRound3", len(shares)*s.Beta(), noise)
	s.in(u, sk)
	call(func() C.int { return C.lr_setup_rkg_round3(s.h, round2.d, u.d, sk.d, bytePtr(noise), C.int(len(shares)), keyHandles(shares)) })
}

// RkgKey = GenRelinearizationKey (:343-355); evkOut may be round2.
func (s *Setup) RkgKey(round2, round3, evkOut *Poly) {
	call(func() C.int { return C.lr_setup_rkg_key(s.h, round2.d, round3.d, evkOut.d) })
}

// RkgNaiveRound1 = RKGProtocolNaive.GenShareRoundOne (dbfv/relinkey_gen_naive.go:59-110; scheme SetupCKKS: dckks/relinkey_gen_naive.go
// with its :73-75): noise [parties][beta][2][N], the planes [parties][beta][N/8].
func (s *Setup) RkgNaiveRound1(scheme int, sk *Poly, pk [2]*Poly, noise, uCoeffs, uSigns []byte, shares []*Poly) {
	s.noiseLen("RkgNaiveRound1", 2*len(shares)*s.Beta(), noise)
	s.planeLen("RkgNaiveRound1", len(shares)*s.Beta(), uCoeffs, uSigns)
	s.in(sk, pk[0], pk[1])
	call(func() C.int {
		return C.lr_setup_rkg_naive_round1(s.h, C.int(scheme), sk.d, pk[0].d, pk[1].d, bytePtr(noise), bytePtr(uCoeffs), bytePtr(uSigns), C.int(len(shares)), keyHandles(shares))
	})
}

// RkgNaiveRound2 = GenShareRoundTwo (:135-166): per digit the ternary v is drawn before the two noise polys.
func (s *Setup) RkgNaiveRound2(round1, sk *Poly, pk [2]*Poly, vCoeffs, vSigns, noise []byte, shares []*Poly) {
	s.noiseLen("RkgNaiveRound2", 2*len(shares)*s.Beta(), noise)
	s.planeLen("RkgNaiveRound2", len(shares)*s.Beta(), vCoeffs, vSigns)
	s.in(sk, pk[0], pk[1])
	call(func() C.int {
		return C.lr_setup_rkg_naive_round2(s.h, round1.d, sk.d, pk[0].d, pk[1].d, bytePtr(vCoeffs), bytePtr(vSigns), bytePtr(noise), C.int(len(shares)), keyHandles(shares))
	})
}

// RkgNaiveKey = RKGProtocolNaive.GenRelinearizationKey (:187-200); evkOut may be round2.
func (s *Setup) RkgNaiveKey(round2, evkOut *Poly) {
	call(func() C.int { return C.lr_setup_rkg_naive_key(s.h, round2.d, evkOut.d) })
}

// RtgShare = RTGProtocol.genShare (dbfv/rotkey_gen.go:139-184) for each Galois element, one call for all of them.
func (s *Setup) RtgShare(sk *Poly, galEls []uint64, crp *Poly, noise []byte, shares []*Poly) {
	if len(galEls) != len(shares) {
		panic("cannot RtgShare: one share per Galois element")
	}
	s.noiseLen("RtgShare", len(shares)*s.Beta(), noise)
	s.in(sk)
	call(func() C.int {
		return C.lr_setup_rtg_share(s.h, sk.d, (*C.uint64_t)(unsafe.Pointer(&galEls[0])), C.int(len(shares)), crp.d, bytePtr(noise), keyHandles(shares))
	})
}

// RtgKey = RTGProtocol.Finalize (:205-215): rotKeyOut is a key image.
func (s *Setup) RtgKey(share, crp, rotKeyOut *Poly) {
	call(func() C.int { return C.lr_setup_rtg_key(s.h, share.d, crp.d, rotKeyOut.d) })
}

// Aggregate = every Aggregate* of the four protocols over all of `shares` in their order, over all of Q||P: images of the same batch, or
// plain polys (CKG).  out may be one of the shares.
func (s *Setup) Aggregate(shares []*Poly, out *Poly) {
	s.in(shares...)
	s.out(out)
	n := len(shares)
	raw := C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0))))
	defer C.free(raw)
	arr := polyArray(raw, n)
	for i := range shares {
		arr[i] = shares[i].d
	}
	call(func() C.int { return C.lr_setup_aggregate(s.h, (**C.lr_poly)(raw), C.int(n), out.d) })
	finished(out)
}

// The Device forms: the same bytes in device memory, stream-ordered on contextQ's stream, no host copy and no synchronisation; the
// plain polys must be resident (Poly.Pin).
func (s *Setup) CkgShareDevice(sk, crs *Poly, noise unsafe.Pointer, shareOut *Poly) {
	s.in(sk, crs)
	s.out(shareOut)
	call(func() C.int { return C.lr_setup_ckg_share_device(s.h, sk.d, crs.d, noise, 1, shareOut.d) })
}

func (s *Setup) RkgRound1Device(u, sk, crp *Poly, noise unsafe.Pointer, shares []*Poly) {
	s.in(u, sk)
	call(func() C.int { return C.lr_setup_rkg_round1_device(s.h, u.d, sk.d, crp.d, noise, C.int(len(shares)), keyHandles(shares)) })
}

func (s *Setup) RkgRound2Device(round1, sk, crp *Poly, noise unsafe.Pointer, shares []*Poly) {
	s.in(sk)
	call(func() C.int { return C.lr_setup_rkg_round2_device(s.h, round1.d, sk.d, crp.d, noise, C.int(len(shares)), keyHandles(shares)) })
}

func (s *Setup) RkgRound3Device(round2, u, sk *Poly, noise unsafe.Pointer, shares []*Poly) {
	s.in(u, sk)
	call(func() C.int { return C.lr_setup_rkg_round3_device(s.h, round2.d, u.d, sk.d, noise, C.int(len(shares)), keyHandles(shares)) })
}

func (s *Setup) RkgNaiveRound1Device(scheme int, sk *Poly, pk [2]*Poly, noise, uCoeffs, uSigns unsafe.Pointer, shares []*Poly) {
	s.in(sk, pk[0], pk[1])
	call(func() C.int {
		return C.lr_setup_rkg_naive_round1_device(s.h, C.int(scheme), sk.d, pk[0].d, pk[1].d, noise, uCoeffs, uSigns, C.int(len(shares)), keyHandles(shares))
	})
}

func (s *Setup) RkgNaiveRound2Device(round1, sk *Poly, pk [2]*Poly, vCoeffs, vSigns, noise unsafe.Pointer, shares []*Poly) {
	s.in(sk, pk[0], pk[1])
	call(func() C.int {
		return C.lr_setup_rkg_naive_round2_device(s.h, round1.d, sk.d, pk[0].d, pk[1].d, vCoeffs, vSigns, noise, C.int(len(shares)), keyHandles(shares))
	})
}

func (s *Setup) RtgShareDevice(sk *Poly, galEls []uint64, crp *Poly, noise unsafe.Pointer, shares []*Poly) {
	s.in(sk)
	call(func() C.int {
		return C.lr_setup_rtg_share_device(s.h, sk.d, (*C.uint64_t)(unsafe.Pointer(&galEls[0])), C.int(len(shares)), crp.d, noise, keyHandles(shares))
	})
}
