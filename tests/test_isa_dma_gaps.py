"""ISA audit of the LDS-DMA gaps in the GEMM K loops (CPU: hipcc cross-compiles).

With one wave per SIMD the K loop issues in order, and an MFMA gap that
carries an LDS-DMA piece (``buffer_load_dwordx4 ... lds``) already runs past
the MFMA's 16 cycles: every further scalar instruction in that gap costs its
whole issue time.  The K-tiles therefore write M0 (the piece's LDS address)
in an MFMA gap AHEAD of the piece (mxk::m0_put) and issue the piece bare
(mxk::dma16q): no ``s_nop``, no M0 write beside it.  M0 is nobody else's in
these loops, which is what lets the two halves stand apart; this file proves
it from the listing.

Audited: the steady-state K loop of TN schedule 52 (six one-barrier K-tiles)
and of every production layout kernel (two three-barrier K-tiles).
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PIECE = re.compile(r"^buffer_load_dwordx4 .*\blds\b")
M0_WRITE = re.compile(r"^s_\w+\s+m0\b")
# a fragment is one ds_read_b128 (K-major image) or two transposed 8-byte reads
FRAG_READS = {"ds_read_b128": 2, "ds_read_b64_tr_b16": 1}


def _asm(src: str, out: str) -> str:
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-I" + os.path.join(REPO, "native", "kernels"), "--cuda-device-only", "-S",
                    os.path.join(REPO, "native", "kernels", src), "-o", out],
                   check=True, capture_output=True)
    with open(out) as f:
        return f.read()


def kernels(asm: str) -> dict[str, list[str]]:
    """Kernel name -> its lines (labels and comments kept)."""
    out = {}
    for name in re.findall(r"^(_Z[^\s:]+):", asm, re.M):
        i = asm.find(name + ":")
        out[name] = asm[i:asm.find(".Lfunc_end", i)].split("\n")
    return out


def steady_loops(lines: list[str]) -> list[list[str]]:
    """Instruction lists of the loops that hold at least one whole K-tile with
    DMA (128 MFMAs and a piece): from a loop header label to the last branch
    back to it (linear layout: LLVM keeps a loop's blocks contiguous)."""
    out = []
    for k, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):.*Loop Header", ln)
        if not m:
            continue
        ends = [e for e in range(k + 1, len(lines))
                if re.match(r"\s*s_c?branch\S*\s+" + re.escape(m.group(1)) + r"\b", lines[e])]
        if not ends:
            continue
        body = [x.split(";")[0].strip() for x in lines[k + 1:ends[-1] + 1]]
        body = [x for x in body if x and not x.startswith(".") and not x.endswith(":")]
        if sum(x.startswith("v_mfma") for x in body) >= 128 and any(PIECE.match(x) for x in body):
            out.append(body)
    return out


def census(loop: list[str]) -> dict[str, int]:
    op = [x.split(" ")[0] for x in loop]
    return {"mfma": sum(o.startswith("v_mfma") for o in op),
            "frag_reads_x2": sum(FRAG_READS.get(o, 0) for o in op),
            "pieces": sum(bool(PIECE.match(x)) for x in loop),
            "m0_writes": sum(bool(M0_WRITE.match(x)) for x in loop),
            "barriers": op.count("s_barrier"),
            "scratch": sum(o.startswith("scratch_") for o in op)}


def gaps(loop: list[str]) -> list[list[str]]:
    """The instructions between consecutive MFMAs (the loop's head before its
    first MFMA and its tail after the last one are gaps too)."""
    out = [[]]
    for x in loop:
        if x.startswith("v_mfma"):
            out.append([])
        else:
            out[-1].append(x)
    return out


def gap_faults(loop: list[str]) -> list[str]:
    """(b) an ``s_nop`` or an M0 write in the MFMA gap of a piece; (c) a piece
    not preceded by exactly one M0 write since the previous piece, or with
    that write right in front of it (the M0 -> LDS-DMA wait state must be a
    real instruction)."""
    bad = []
    for g in gaps(loop):
        if any(PIECE.match(x) for x in g):
            bad += ["filler beside a piece: " + x for x in g
                    if x.startswith("s_nop") or M0_WRITE.match(x)]
    writes, last_write = 0, None
    for n, x in enumerate(loop):
        if M0_WRITE.match(x):
            writes, last_write = writes + 1, n
        elif PIECE.match(x):
            if writes != 1:
                bad.append("%d M0 writes before piece %d: %s" % (writes, n, x))
            elif n - last_write < 2:
                bad.append("no instruction between the M0 write and piece %d: %s" % (n, x))
            writes = 0
    if writes:
        bad.append("%d M0 writes after the last piece" % writes)
    return bad


def check_loop(loop: list[str], barriers_per_ktile: int) -> None:
    c = census(loop)
    kt = c["mfma"] // 128
    assert c == {"mfma": 128 * kt, "frag_reads_x2": 64 * kt, "pieces": 16 * kt,
                 "m0_writes": 16 * kt, "barriers": barriers_per_ktile * kt, "scratch": 0}, c
    assert gap_faults(loop) == []


def test_detector_on_a_hand_written_k_loop():
    mfma = "v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]"
    piece = "buffer_load_dwordx4 v9, s[8:11], s14 offen lds"
    good = [mfma, "s_mov_b32 m0, s20", mfma, piece, mfma, "ds_read_b128 v[0:3], v8",
            "s_add_u32 m0, s20, 0x400", mfma, "ds_read_b128 v[4:7], v8 offset:64", piece, mfma]
    assert gap_faults(good) == []
    assert census(good)["m0_writes"] == 2 and census(good)["pieces"] == 2
    # the parent's form: nop, piece and the next piece's M0 write in one gap
    old = [mfma, "s_nop 0", piece, "s_mov_b32 m0, s21", mfma, "s_nop 0", piece,
           "s_mov_b32 m0, s22", mfma]
    f = gap_faults(old)
    assert sum("filler beside a piece" in x for x in f) == 4
    assert any("0 M0 writes before piece" in x for x in f)
    # the write right in front of its piece, though in the gap before
    assert gap_faults([mfma, "s_mov_b32 m0, s20", piece, mfma]) != []
    close = [mfma, "s_mov_b32 m0, s20", mfma, piece, mfma]
    assert gap_faults(close) == []
    assert any("no instruction between" in x
               for x in gap_faults(["s_mov_b32 m0, s20", piece, mfma]))
    # a second writer of M0 (a save / restore pair, the compiler's own use)
    twice = [mfma, "s_mov_b32 m0, s20", mfma, "s_mov_b32 m0, s3", mfma, piece, mfma]
    assert any("2 M0 writes" in x for x in gap_faults(twice))
    # the loop finder: header label to the branch back, comments dropped
    text = ["_Zk:", ".LBB0_1:  ; =>This Inner Loop Header: Depth=1"] + \
           ["\t" + x + " ; c" for x in [mfma] * 128 + [piece]] + ["\ts_cbranch_scc1 .LBB0_1", mfma]
    (lp,) = steady_loops(text)
    assert census(lp)["mfma"] == 128 and census(lp)["pieces"] == 1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_tn_schedule_52_k_loop_has_bare_pieces(tmp_path):
    """mxk_gemm_bf16_tn_w4k<1, 4, 0, 1>: six one-barrier K-tiles per trip."""
    ks = kernels(_asm("gemm_bf16.hip", str(tmp_path / "tn.s")))
    (name,) = [n for n in ks if "mxk_gemm_bf16_tn_w4kILi1ELi4ELi0ELi1E" in n]
    loops = steady_loops(ks[name])
    assert len(loops) == 1
    assert census(loops[0])["mfma"] == 6 * 128
    check_loop(loops[0], 1)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_layout_k_loops_have_bare_pieces(tmp_path):
    """Every production layout kernel (mxk_gemm_bf16_x2_kernel): the
    three-barrier K-tile, unrolled by two."""
    ks = kernels(_asm("gemm_bf16_layouts.hip", str(tmp_path / "x2.s")))
    names = [n for n in ks if "mxk_gemm_bf16_x2_kernel" in n]
    assert names
    for n in names:
        loops = steady_loops(ks[n])
        assert len(loops) == 1, n
        assert census(loops[0])["mfma"] == 2 * 128, n
        check_loop(loops[0], 3)
