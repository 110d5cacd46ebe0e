"""The catalogue of the assembly NTT code objects: which ones ship, what each is called, how each is generated.

Everything else reads this: build.sh builds `shipped()`, lr_asm.cpp loads the table written here (names and block sizes), the emulator
harness (tests/asm_emulate.py) constructs its generators through `make`.  A new code object is one more entry of `shipped()`.

    python catalogue.py list [--diag]             # the kernel names, in the order of the loader's table
    python catalogue.py build OUTDIR [--diag]     # OUTDIR/ntt_*.s -> .o -> .hsaco, and OUTDIR/lr_asm_blob.cpp

mode (the "_m<mode>" of a name; the host calls it the variant):
    forward  0, 1, 2   the integer kernels Gen(mode): q < 2^61, q <= 2^60, q < 2^57
             3         dual: FP64 body for the limbs below 2^46, the integer body of mode 2 for the others
             4         mode 3 with the subtract-multiply-add epilogue
             5         the integer kernel of mode 1 with the epilogue in integer arithmetic
    inverse  0, 1      the integer kernels GenInv(mode): q < 2^61, q <= 2^60
             3         dual: FP64 body below 2^46, the integer body of mode 1 for the others
tag (degree and flavour), see TAGS; suffix "t": the clock-stamping build (profile) of the same kernel.
"""
import argparse
import os
import subprocess
import sys
from collections import namedtuple
from concurrent.futures import ProcessPoolExecutor

from gen_intt import GenInv
from gen_ntt import Dual, Gen, kernel_text_for

def make(direction, mode, logn, threads=1024, **flavour):
    """the generator of a (direction, mode): the only place that composes Gen / GenInv / Dual.  flavour: sub, profile; forward also
    fused, persist; inverse also fuse_last (anything else is a TypeError of the generator)"""
    if mode not in {"fwd": (0, 1, 2, 3, 4, 5), "inv": (0, 1, 3)}[direction]:
        raise ValueError("no %s kernel of mode %s" % (direction, mode))
    if direction == "inv":
        if mode == 3:
            return Dual(lambda fp: GenInv(logn, 1, threads, fp=fp, dual=True, **flavour))
        return GenInv(logn, mode, threads, **flavour)
    if mode in (3, 4):
        return Dual(lambda fp: Gen(logn, 2, threads, fp=fp, dual=True, epi=mode == 4, **flavour))
    if mode == 5:
        return Gen(logn, 1, threads, epi=True, **flavour)
    return Gen(logn, mode, threads, **flavour)


def key(direction, mode, logn, threads=1024, **flavour):
    """the arguments of `make` as one string: what a kernel and an emulator case compare (so neither spells out a generator's default)"""
    extra = ["%s=%s" % (k, v) for k, v in sorted(flavour.items())]
    return " ".join(["%s mode=%d logn=%d threads=%d" % (direction, mode, logn, threads)] + extra)


# tag -> (logn of the generator, flavour forward, flavour inverse); None: no such kernel in that direction
TAGS = {
    "14": (14, {}, {}), "15": (15, {}, {}),                                   # one 1024-thread workgroup per transform
    "12x": (12, {}, {}), "13x": (13, {}, {}), "14x": (14, {}, {}),            # fewer threads, several workgroups per CU (PLAN)
    # N = 2^16 as two 2^15 sub-blocks.  Forward: "s" the top stage fused into the loads, "p" plain (after ntt_top_kernel or a producer
    # that applied it).  Inverse: "s" lazy outputs (ntt_top_kernel follows), "f" the last stage by the second finisher of each pair
    "16s": (15, {"sub": True}, {"sub": True}),
    "16p": (15, {"sub": True, "fused": False}, None),
    "16f": (15, None, {"sub": True, "fuse_last": True}),
    # N = 2^15 as two 2^14 sub-blocks (launches too small to fill the chip): plain forward, lazy inverse
    "15h": (14, {"sub": True, "fused": False}, {"sub": True}),
    "15p": (15, {"persist": True}, None),                                     # diagnostics: several polys per workgroup
}
# measured best block size of the "x" kernels per degree and direction; everything else runs 1024 threads
PLAN = {("fwd", "12x"): 256, ("inv", "12x"): 256, ("fwd", "13x"): 256, ("inv", "13x"): 512, ("fwd", "14x"): 512, ("inv", "14x"): 512}


class Kernel(namedtuple("Kernel", "direction tag mode suffix diag", defaults=("", False))):
    @property
    def stem(self):
        return "%s%s_m%d%s" % (self.direction, self.tag, self.mode, self.suffix)

    @property
    def name(self):                   # lr_asm.cpp (launch_ntt_asm, launch_ntt_asm16) formats the same name at run time
        return "lr_ntt_" + self.stem

    @property
    def threads(self):
        return PLAN.get((self.direction, self.tag), 1024)

    @property
    def args(self):
        """(direction, mode, logn, threads), flavour: the arguments of `make` and `key`"""
        logn, fwd, inv = TAGS[self.tag]
        flavour = fwd if self.direction == "fwd" else inv
        if flavour is None or self.suffix not in ("", "t"):
            raise ValueError("no kernel " + self.name)
        return (self.direction, self.mode, logn, self.threads), dict(flavour, **({"profile": True} if self.suffix else {}))

    def key(self):
        a, flavour = self.args
        return key(*a, **flavour)

    def generator(self):
        a, flavour = self.args
        return make(*a, **flavour)

    def text(self):
        return kernel_text_for(self.generator(), self.name)


def shipped(diag=False):
    """the code objects of the library, in the order of lr_asm_blobs[]; diag: with those of the diagnostics build (LR_BUILD_DIAG)"""
    whole, fx, ix = ("14", "15"), ("12x", "13x", "14x", "16s", "16p"), ("12x", "13x", "14x", "16s", "16f")
    ks = [Kernel("fwd", t, m) for t in whole for m in (0, 1, 2)] + [Kernel("inv", t, m) for t in whole for m in (0, 1)]
    ks += [Kernel("fwd", t, m) for t in fx for m in (0, 1, 2)] + [Kernel("inv", t, m) for t in ix for m in (0, 1)]
    ks += [Kernel("fwd", t, 3) for t in whole + fx] + [Kernel("inv", t, 3) for t in whole + ix]
    ks += [Kernel("fwd", t, m) for m in (4, 5) for t in whole + fx]
    if diag:
        # the 2^15 kernels with per-phase clock stamps (tools/timeline.py); the persistent forward kernels and their stamped builds
        ks += [Kernel(d, "15", m, "t", True) for d in ("fwd", "inv") for m in (1, 3)]
        ks += [Kernel("fwd", "15p", m, "", True) for m in (0, 1, 2, 3)] + [Kernel("fwd", "15p", m, "t", True) for m in (1, 3)]
    ks += [Kernel("fwd", "15h", m) for m in (0, 1, 2, 3, 4, 5)] + [Kernel("inv", "15h", m) for m in (0, 1, 3)]
    return ks


def _build_one(job):
    k, outdir, llvm = job
    base = os.path.join(outdir, "ntt_" + k.stem)
    with open(base + ".s", "w") as f:
        f.write(k.text())
    for cmd in ([llvm + "/clang", "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", base + ".s", "-o", base + ".o"],
                [llvm + "/ld.lld", "-shared", base + ".o", "-o", base + ".hsaco"]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            return "%s: %s failed (%d)\n%s" % (k.name, " ".join(cmd), r.returncode, r.stderr)
    return None


def build(outdir, diag):
    ks = shipped(diag)
    llvm = os.environ.get("LLVM", "/opt/rocm/lib/llvm/bin")
    os.makedirs(outdir, exist_ok=True)
    with ProcessPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as pool:
        errors = [e for e in pool.map(_build_one, [(k, outdir, llvm) for k in ks]) if e]
    if errors:
        sys.exit("\n".join(errors))
    out = ["struct lr_asm_blob { const char *name; const unsigned char *data; unsigned long size; unsigned threads; };"]
    for k in ks:
        data = open(os.path.join(outdir, "ntt_%s.hsaco" % k.stem), "rb").read()
        out.append("static const unsigned char blob_%s[] __attribute__((aligned(4096))) = {" % k.stem)
        out.append(",".join(str(b) for b in data))
        out.append("};")
    out.append('extern "C" const lr_asm_blob lr_asm_blobs[] = {')
    for k in ks:
        out.append('  {"%s", blob_%s, sizeof(blob_%s), %d},' % (k.name, k.stem, k.stem, k.threads))
    out.append("};")
    out.append('extern "C" const int lr_asm_blob_count = %d;' % len(ks))
    with open(os.path.join(outdir, "lr_asm_blob.cpp"), "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("command", choices=("list", "build"))
    ap.add_argument("outdir", nargs="?")
    ap.add_argument("--diag", action="store_true", default=bool(os.environ.get("LR_BUILD_DIAG")))
    args = ap.parse_args()
    if args.command == "list":
        print("\n".join(k.name for k in shipped(args.diag)))
    elif not args.outdir:
        ap.error("build needs OUTDIR")
    else:
        build(args.outdir, args.diag)
