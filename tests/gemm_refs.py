"""Inputs, frames and fp64 references for the GEMM placement tests, shared by tests/test_gemm_refs_cpu.py (no GPU: the reference passes
its own gates, every wrong kernel written in torch is rejected by a named case) and tests/test_gemm_frames_gpu.py (the HIP kernels).

What the tests of tests/test_ops_gpu.py cannot see and these can:
  * every operand is a VIEW: A = columns [64, 64 + K) of rows of K + 128 (+ a per-group extra) elements, C = [0:M, 64:64 + N] of a frame of
    ceil(M / 256) * 256 + 256 rows of N + 128 elements, resid either a separate buffer with ldr = N + 64 or C itself, the split's fp8 half at
    c2_col0 = 128 of rows of 128 + (N - split_n) + 64 bytes.  All strides, offsets and bases are multiples of 64 bytes;
  * everything outside a view is a sentinel: NaN in the operand's format around A and resid (a read of a gap poisons the result), the
    bf16 NaN payload 0x7FC1 / the byte 0xFE around C / C2, compared bit for bit after the launch.  The C frame is taller than any tile that
    covers row M - 1, so a store that is not masked lands IN the frame and is reported;
  * every launcher meets fp64, at M in {1, bm - 1, bm, bm + 1}, at K from the minimum through two K-steps past the kernel's ring, at
    tile counts around its band height, with two and three groups, groups without bias, and groups of no rows.

The reference is fp64 on the identical quantised operands, rounded once to bf16; gate*y+x follows test_ops_gpu.py::test_gemm_split_k.  The
gates are the project's: assert_close_mag(mag=accum_noise, ulps=1.05, min_exact=0.98), and ulps=2.05, min_exact=0.95 for gate*y+x.
min_exact needs a population: cases of fewer than POOL outputs are repeated with fresh seeds and gated together."""
import zlib
from collections import namedtuple

import torch

import flux_oracle as fo
from parity_util import accum_noise, assert_close_mag, round_fp64_to_bf16

E4M3, E5M2 = 0, 1
F8T = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
F8MAX = {E4M3: 448.0, E5M2: 57344.0}
EPI_BF16, EPI_GATE_RESID, EPI_SPLIT = 0, 2, 3
EPI_ID = {"plain": EPI_BF16, "gate": EPI_GATE_RESID, "split": EPI_SPLIT}
SENTINEL = 0x7FC1  # bf16 NaN payload no kernel produces
SENT8 = 0xFE       # fp8 output frames (a NaN of e5m2; the quantising epilogue clamps, it never stores one)
NAN8 = 0x7F        # NaN in both fp8 formats: the gaps of fp8 operands
POOL = 4096        # min_exact is gated on at least this many outputs
C2_COL0 = 128
GENERIC, AUTO, SPLITK0 = 100, -1, 113  # tile_cfg: the generic kernel, the planner, split-K with S slices = SPLITK0 + S

# Restated from csrc/gemm_cfg.h (bm, bn, K-step bytes, minimum K bytes) and from the launchers: `band` = group_m, the row tiles of one band
# of the rasterisation (gemm.hip / gemm_pp.hip: 8, gemm_w1.hip W1_GROUP_M: 6, gemm_persist.hip PS_GROUP_M: 4); `ksteps` = the K-step counts
# that walk the kernel's pipeline from its minimum through two steps past its depth, plus an odd count of 17:
#   gemm.hip      2 LDS buffers of 128-byte steps, one staged ahead                       -> 1 .. 4
#   gemm_pp.hip   4-slot ring of 64-byte steps, 3 in flight (prologue nk > 1, nk > 2)      -> 1 .. 6
#   gemm_w1.hip   4-slot ring of 64-byte steps walked four at a time (one 256-byte step)   -> 1 .. 3
#   gemm_persist  5-slot ring of 64-byte steps, 4 in flight, the slot of a tile's first step advances by nk % 5 per tile: 2, 3, 4, 5 and
#                 6 steps of 256 bytes are nk = 8, 12, 16, 20, 24, i.e. every residue 3, 2, 1, 0, 4 (past K = 1024: the ring asks for it)
#   generic       no pipeline, 16-byte pieces: steps of 64 bytes keep every stride a multiple of 64 bytes
TILES = {
    2: dict(bm=128, bn=128, kstep=128, min_k=128, band=8, ksteps=(1, 2, 3, 4, 17)),
    15: dict(bm=128, bn=64, kstep=128, min_k=128, band=8, ksteps=(1, 2, 3, 4, 17)),
    13: dict(bm=256, bn=256, kstep=64, min_k=64, band=8, ksteps=(1, 2, 3, 4, 5, 6, 17)),
    16: dict(bm=256, bn=256, kstep=256, min_k=256, band=6, ksteps=(1, 2, 3, 17)),
    17: dict(bm=192, bn=256, kstep=256, min_k=256, band=6, ksteps=(1, 2, 3, 17)),
    20: dict(bm=224, bn=256, kstep=256, min_k=256, band=6, ksteps=(1, 2, 3, 17)),
    21: dict(bm=160, bn=256, kstep=256, min_k=256, band=6, ksteps=(1, 2, 3, 17)),
    18: dict(bm=256, bn=256, kstep=256, min_k=512, band=4, ksteps=(2, 3, 4, 5, 6, 17)),
    GENERIC: dict(bm=16, bn=16, kstep=64, min_k=64, band=0, ksteps=(1, 2, 3, 17)),
    SPLITK0 + 2: dict(bm=256, bn=256, kstep=64, min_k=128, band=8, ksteps=()),
}
# operand format x epilogue every launcher is compiled for (gemm_cfg.h GemmTakes, fluxmi_gemm_persist_ok, launch_pp_splitk)
ANY = (("f8", "plain"), ("f8", "gate"), ("bf16", "plain"), ("bf16", "gate"))
TAKES = {2: ANY, 15: ANY, 13: ANY, 16: ANY, GENERIC: ANY, SPLITK0 + 2: ANY, 17: (("f8", "gate"), ("bf16", "plain"), ("bf16", "gate")),
         20: (("f8", "gate"),), 21: (("f8", "gate"),), 18: (("f8", "plain"), ("f8", "gate"), ("f8", "split"))}
LAUNCHERS = (2, 15, 13, 16, 17, 18, 20, 21, GENERIC, SPLITK0 + 2)

Case = namedtuple("Case", "id cfg op fmt epi N K Ms bias lda_extra resid split_n")


def launcher_name(cfg):
    return "auto" if cfg == AUTO else "generic" if cfg == GENERIC else f"splitk{cfg - SPLITK0}" if cfg > SPLITK0 else f"cfg{cfg}"


def n_of(cfg):
    return {2: 128, 15: 64}.get(cfg, 256)


def _case(family, cfg, op, epi, Ms, N, kbytes, fmt=E5M2, bias=None, lda_extra=None, resid=None):
    Ms = tuple(Ms)
    K = kbytes if op == "f8" else kbytes // 2
    if resid is None:  # the separate and the in-place residual take turns
        resid = ("sep", "inplace")[(sum(Ms) + len(Ms)) % 2] if epi == "gate" else None
    bias = tuple(bias) if bias is not None else (True,) * len(Ms)
    lda_extra = tuple(lda_extra) if lda_extra is not None else (0,) * len(Ms)
    split_n = N // 2 if epi == "split" else 0
    name = f"{launcher_name(cfg)}-{op}{'-e4m3' if (op == 'f8' and fmt == E4M3) else ''}-{epi}{'-' + resid if resid else ''}-{family}-M{'_'.join(map(str, Ms))}-N{N}-K{K}"
    if not all(bias):
        name += "-bias" + "".join("1" if b else "0" for b in bias)
    return Case(name, cfg, op, fmt, epi, N, K, Ms, bias, lda_extra, resid, split_n)


def _cases():
    out = []
    for cfg in LAUNCHERS:
        t, N = TILES[cfg], n_of(cfg)
        bm = t["bm"]
        first = TAKES[cfg][0]
        # ---- M edges: one row, one short of a tile, a tile, a tile and a row; every operand format x epilogue of the launcher
        for op, epi in TAKES[cfg]:
            for M in (1, bm - 1, bm, bm + 1):
                out.append(_case("m", cfg, op, epi, [M], 512 if epi == "split" else N, 512))
        # ---- bands: row tiles = band - 1, band, band + 1 (ragged last tile), two column tiles; 11 x 2 tiles: not a multiple of the 8 XCDs
        if t["band"]:
            for tiles in (t["band"] - 1, t["band"], t["band"] + 1, 11):
                out.append(_case("band" if tiles != 11 else "xcd", cfg, first[0], first[1], [tiles * bm - 5], 2 * N, 512))
        # ---- K edges (two row tiles, the second of one row)
        ops_k = [first] + ([("bf16", "plain")] if cfg in (2, 13, 16, 17, GENERIC) and first != ("bf16", "plain") else [])
        for op, epi in ops_k:
            for steps in t["ksteps"]:
                out.append(_case(f"k{steps}", cfg, op, epi, [bm + 1], N, steps * t["kstep"]))
        # ---- groups: own A, W, bias and scales each; a group without bias behind one with; an own lda each (the persistent kernel: one lda);
        # an empty group first, in the middle, last
        ex = (0, 0, 0) if cfg == 18 else (0, 64, 128)
        gate = ("f8", "gate") in TAKES[cfg]
        plain = ("f8", "plain") in TAKES[cfg]
        for family, Ms, bias, epi in (("mixed", (bm + 1, 1, 77), (1, 0, 1), "gate"), ("two", (bm + 1, 77), (1, 0), "plain"),
                                      ("empty0", (0, bm + 1, 77), (1, 1, 0), "gate"), ("empty1", (bm + 1, 0, 77), (1, 0, 1), "plain"),
                                      ("empty2", (bm + 1, 77, 0), (0, 1, 1), "gate")):
            epi = epi if (epi == "gate" and gate) or (epi == "plain" and plain) else ("gate" if gate else "plain")
            out.append(_case(family, cfg, "f8", epi, Ms, N, 512, bias=bias, lda_extra=ex[:len(Ms)]))
        if cfg in (2, 13, 16, 17):
            out.append(_case("mixed", cfg, "bf16", "gate", (bm + 1, 1, 77), N, 512, bias=(1, 0, 1), lda_extra=ex))
    # fp8 e4m3 activations once on each kernel file's fp8 path
    for cfg in (2, 13, 16):
        out.append(_case("m", cfg, "f8", "plain", [TILES[cfg]["bm"] + 1], n_of(cfg), 512, fmt=E4M3))
    # the persistent kernel's split: the bf16 half in one frame, the fp8 half (through the table) in another, table and plain tiles in one launch
    out.append(_case("mixed", 18, "f8", "split", (257, 1, 77), 512, 512, bias=(1, 0, 1)))
    out.append(_case("empty1", 18, "f8", "split", (257, 0, 77), 512, 768, bias=(1, 1, 0)))
    # split-K: 7 K-steps over 3 slices (2 + 2 + 3) and exactly one step per slice
    for op, epi in ANY:
        for steps in (7, 3):
            out.append(_case(f"k{steps}", SPLITK0 + 3, op, epi, [257], 256, steps * 64))
    # the planner's own choice on a few of the same cases
    for op, epi, Ms, N, kb, bias, ex in (("f8", "plain", (257,), 256, 512, None, None), ("bf16", "gate", (255,), 256, 512, None, None),
                                         ("f8", "plain", (129,), 128, 384, None, None), ("f8", "gate", (257, 1, 77), 256, 512, (1, 0, 1), (0, 64, 128)),
                                         ("f8", "plain", (257, 0, 77), 256, 512, (1, 0, 1), (0, 64, 128)), ("bf16", "plain", (1,), 64, 128, None, None)):
        out.append(_case("auto", AUTO, op, epi, Ms, N, kb, bias=bias, lda_extra=ex))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def outputs_of(case):
    return sum(case.Ms) * (case.split_n if case.epi == "split" else case.N)


def pool_reps(case):
    """repetitions with fresh seeds that bring a case to POOL outputs"""
    return max(1, -(-POOL // outputs_of(case)))


# ---- operands and the fp64 reference -------------------------------------------------------------------------------------------------
def make_problem(case, rep=0):
    """per group: quantised operands (as make_f8_problem / test_bf16_gemm build them: asymmetric data, one scaled weight row, per-tensor
    scales), bias or None, gate, residual, and the fp64 reference with its magnitude for assert_close_mag"""
    g = torch.Generator().manual_seed((zlib.crc32(case.id.encode()) + 7919 * rep) % (2 ** 31))
    N, K, groups = case.N, case.K, []
    for gi, M in enumerate(case.Ms):
        if case.op == "f8":
            a = (torch.randn(M, K, generator=g) * 2.0).bfloat16()
            w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
            a[:, 3] += 1.5
            w[1] *= 3.0
            sa = fo.amax_to_scale(a.abs().max().float() if M else torch.tensor(1.0), F8MAX[case.fmt])
            a = fo.to_fp8_saturated(a, sa, F8MAX[case.fmt]).to(F8T[case.fmt])
            w, _, sbr = fo.quantize_weight(w)
            sar = sa.reciprocal()
            sc = (sar * sbr).float()
        else:
            a = torch.randn(M, K, generator=g).bfloat16()
            w = (torch.randn(N, K, generator=g) * 0.1).bfloat16()
            a[:, 1] += 2
            sar = sbr = None
            sc = torch.tensor(1.0)
        bias = torch.randn(N, generator=g).bfloat16() if case.bias[gi] else None
        gate = torch.randn(N, generator=g).bfloat16() if case.epi == "gate" else None
        x = torch.randn(M, N, generator=g).bfloat16() if case.epi == "gate" else None
        p = dict(M=M, a=a, w=w, bias=bias, gate=gate, x=x, sar=sar, sbr=sbr, sc=sc)
        p["ref"], p["mag"] = reference(case, p, a.double() @ w.double().T)
        groups.append(p)
    return groups


def reference(case, p, acc):
    """(bf16 reference, magnitude) from the accumulators `acc` (fp64: THE reference; fp32: the emulation whose distance the gates allow)"""
    b = p["bias"].double() if p["bias"] is not None else 0.0
    h = round_fp64_to_bf16(acc.double() * p["sc"].double() + b)
    noise = accum_noise(p["a"], p["w"], float(p["sc"]))
    if case.epi == "gate":  # test_ops_gpu.py::test_gemm_split_k
        gate, x = p["gate"], p["x"]
        ref = (x.float() + (gate.float() * h.float()).bfloat16().float()).bfloat16()
        gh = (gate.float() * h.float()).abs().double()
        return ref, torch.maximum(torch.maximum(noise * gate.float().abs()[None, :].double(), gh), x.double().abs())
    if case.epi == "split":
        return h[:, :case.split_n].contiguous(), noise[:, :case.split_n]
    return h, noise


def gate_of(case):
    return dict(ulps=2.05, min_exact=0.95) if case.epi == "gate" else dict(ulps=1.05, min_exact=0.98)


# ---- frames --------------------------------------------------------------------------------------------------------------------------
def _nan_fill(shape, dtype):
    if dtype == torch.bfloat16:
        return torch.full(shape, SENTINEL, dtype=torch.int16).view(torch.bfloat16)
    return torch.full(shape, NAN8, dtype=torch.uint8).view(dtype)


def make_frames(case, prob, device="cpu", dense=False, c_off=64, c_pad=128):
    """per group: flat buffers + (offset, stride) of every view, as the kernels address them.  dense=True: the same operands with
    lda == K, ldc == N, ldr == N, c2_col0 == 0 and no frame; c_off / c_pad: another column offset and row padding of the C view.
    Buffers live on `device`; the `keep` masks (CPU) mark the bytes a launch may write."""
    N, K = case.N, case.K
    Nc = case.split_n if case.epi == "split" else N
    frames = []
    for gi, p in enumerate(prob):
        M = p["M"]
        f = dict(M=M)
        # A: [M + 1 rows][lda]; the view's last row is followed by the rest of its row and one spare row, because the descriptor kernels may
        # fetch (and drop) up to lda - K elements behind it (include/fluxmi.h)
        lda, a_off = (K, 0) if dense else (K + 128 + case.lda_extra[gi], 64)
        a_buf = _nan_fill((M + 1, lda), p["a"].dtype)
        a_buf[:M, a_off:a_off + K] = p["a"]
        f.update(a_buf=a_buf.reshape(-1).to(device), a_off=a_off, lda=lda)
        # C (bf16): tall frame, view [0:M, 64:64 + Nc]
        rows = max(M, 1) if dense else (M + 255) // 256 * 256 + 256
        ldc, c_off = (Nc, 0) if dense else (Nc + c_pad, c_off)
        c_buf = torch.full((rows, ldc), SENTINEL, dtype=torch.int16)
        keep = torch.zeros(rows, ldc, dtype=torch.bool)
        keep[:M, c_off:c_off + Nc] = True
        f.update(c_rows=rows, c_off=c_off, ldc=ldc, c_keep=keep.reshape(-1))
        if case.epi == "gate":
            if case.resid == "inplace":
                c_buf[:M, c_off:c_off + Nc] = p["x"].view(torch.int16)
                f.update(r_buf=None, r_off=c_off, ldr=ldc)
            else:
                ldr = N if dense else N + 64
                r_buf = _nan_fill((max(M, 1), ldr), torch.bfloat16)
                r_buf[:M, :N] = p["x"]
                f.update(r_buf=r_buf.reshape(-1).to(device), r_off=0, ldr=ldr, r_orig=r_buf.reshape(-1).view(torch.int16).clone())
        f["c_buf"] = c_buf.reshape(-1).view(torch.bfloat16).to(device)
        if case.epi == "split":
            n2 = N - case.split_n
            ldc2, col0 = (n2, 0) if dense else (C2_COL0 + n2 + 64, C2_COL0)
            keep2 = torch.zeros(rows, ldc2, dtype=torch.bool)
            keep2[:M, col0:col0 + n2] = True
            f.update(c2_buf=torch.full((rows * ldc2,), SENT8, dtype=torch.uint8).to(device), ldc2=ldc2, c2_col0=col0, c2_keep=keep2.reshape(-1))
        frames.append(f)
    return frames


def view_c(case, f):
    """the C view of a frame as a [M, Nc] bf16 CPU tensor"""
    Nc = case.split_n if case.epi == "split" else case.N
    return f["c_buf"].cpu().view(f["c_rows"], f["ldc"])[:f["M"], f["c_off"]:f["c_off"] + Nc].contiguous()


def view_c2(case, f):
    n2 = case.N - case.split_n
    return f["c2_buf"].cpu().view(f["c_rows"], f["ldc2"])[:f["M"], f["c2_col0"]:f["c2_col0"] + n2].contiguous()


def frame_damage(case, frames):
    """every sentinel of every frame, bit for bit: a list of complaints (empty = intact)"""
    bad = []
    for gi, f in enumerate(frames):
        c = f["c_buf"].cpu().view(torch.int16)
        hit = (~f["c_keep"]) & (c != SENTINEL)
        if hit.any():
            idx = hit.nonzero()[:4, 0]
            bad.append(f"group {gi}: {int(hit.sum())} words of the C frame overwritten, first (row, col) {[(int(i) // f['ldc'], int(i) % f['ldc']) for i in idx]} (view: rows < {f['M']}, cols {f['c_off']}..)")
        if f.get("r_buf") is not None and not torch.equal(f["r_buf"].cpu().view(torch.int16), f["r_orig"]):
            bad.append(f"group {gi}: the separate residual buffer was written")
        if "c2_buf" in f:
            c2 = f["c2_buf"].cpu()
            hit = (~f["c2_keep"]) & (c2 != SENT8)
            if hit.any():
                idx = hit.nonzero()[:4, 0]
                bad.append(f"group {gi}: {int(hit.sum())} bytes of the C2 frame overwritten, first (row, col) {[(int(i) // f['ldc2'], int(i) % f['ldc2']) for i in idx]}")
    return bad


# ---- the kernel, written in torch on the same frames (CPU): correct, or wrong in one named way ------------------------------------------
MUTANTS = ("a_dense", "c_dense", "ldr_is_ldc", "row_at_M", "full_n_tile", "group0_w", "group0_bias", "group0_scale", "drop_last_kstep",
           "splitk_late", "ignore_c2_col0")


def emulate(case, prob, frames, mutant=None):
    """What a kernel does to the frames, with fp32 accumulation (torch's fp32 matmul) and ONE rounding of h: loads and stores go through flat
    (base + row * stride + column) indices like the kernels'.  `mutant` breaks one thing (MUTANTS)."""
    N, K = case.N, case.K
    eb = 1 if case.op == "f8" else 2
    for gi, (p, f) in enumerate(zip(prob, frames)):
        M = f["M"]
        if M == 0:
            continue
        src = prob[0] if gi == 1 else p
        w = src["w"] if mutant == "group0_w" else p["w"]
        bias = src["bias"] if mutant == "group0_bias" else p["bias"]
        sc = src["sc"] if mutant == "group0_scale" else p["sc"]
        lda = K if mutant == "a_dense" else f["lda"]
        rows, ks = torch.arange(M), torch.arange(K)
        raw = torch.uint8 if eb == 1 else torch.int16  # (indexing goes through integer views: the bytes are what moves)
        a = f["a_buf"].view(raw)[f["a_off"] + rows[:, None] * lda + ks[None, :]].view(p["a"].dtype).float()
        wf = w.float()
        step = 64 // eb  # elements of a 64-byte K-step
        if mutant == "drop_last_kstep":
            a, wf = a[:, :K - step], wf[:, :K - step]
        if mutant == "splitk_late" and case.cfg > SPLITK0:
            S, nk = case.cfg - SPLITK0, K // step
            live = torch.ones(K, dtype=torch.bool)
            for s in range(1, S):
                k0 = s * nk // S
                live[k0 * step:(k0 + 1) * step] = False
            a, wf = a[:, live], wf[:, live]
        acc = a @ wf.T
        b = bias.double() if bias is not None else 0.0
        h = round_fp64_to_bf16(acc.double() * sc.double() + b)
        cols = torch.arange(N)
        ldc = (case.split_n if case.epi == "split" else N) if mutant == "c_dense" else f["ldc"]
        if case.epi == "gate":
            rb = f["r_buf"] if f["r_buf"] is not None else f["c_buf"]
            ldr = ldc if mutant == "ldr_is_ldc" else f["ldr"]
            x = rb.view(torch.int16)[(f["r_off"] + rows[:, None] * ldr + cols[None, :]).clamp(max=rb.numel() - 1)].view(torch.bfloat16)
            out = (x.float() + (p["gate"].float() * h.float()).bfloat16().float()).bfloat16()
        else:
            out = h
        Nc = case.split_n if case.epi == "split" else N
        m_idx, vals = rows, out[:, :Nc]
        if mutant == "row_at_M":  # the tile's next row is stored as well (computed from the clamped last row, as a padded row would be)
            m_idx, vals = torch.arange(M + 1), torch.cat([vals, vals[-1:]])
        n_idx = torch.arange(Nc)
        if mutant == "full_n_tile" and Nc % 256:  # a whole 256-column tile although the launch has fewer columns
            n_idx = torch.arange((Nc + 255) // 256 * 256)
            vals = torch.cat([vals, torch.zeros(vals.shape[0], len(n_idx) - Nc, dtype=vals.dtype)], 1)
        f["c_buf"].view(torch.int16)[f["c_off"] + m_idx[:, None] * ldc + n_idx[None, :]] = vals.contiguous().view(torch.int16)
        if case.epi == "split":  # placement only: any deterministic byte per element stands for the quantised GELU
            n2 = N - case.split_n
            q = (h[:, case.split_n:].contiguous().view(torch.int16) & 0x7F).to(torch.uint8)
            col0 = 0 if mutant == "ignore_c2_col0" else f["c2_col0"]
            f["c2_buf"][rows[:, None] * f["ldc2"] + col0 + torch.arange(n2)[None, :]] = q


# ---- gates ---------------------------------------------------------------------------------------------------------------------------
def stats(got, ref, mag, ulps):
    """(worst err / tol, bit-exact share) of the gate assert_close_mag applies"""
    g, r = got.double(), ref.double()
    tol = ulps * torch.maximum(r.abs(), mag.double()) * 2.0 ** -7
    err = (g - r).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return float((err / tol.clamp_min(1e-300)).max()) if g.numel() else 0.0, float((g == r).double().mean()) if g.numel() else 1.0


def run_case(case, launch, device="cpu"):
    """Every repetition of a case: build operands and frames, `launch(case, prob, frames, rep)` (returns complaints of its own), collect the views and check the
    frames; then the pooled views against the pooled fp64 reference through the project's gate.  Returns (worst err / tol, bit-exact share)."""
    got, ref, mag, complaints = [], [], [], []
    for rep in range(pool_reps(case)):
        prob = make_problem(case, rep)
        frames = make_frames(case, prob, device)
        complaints += [f"rep {rep}: {c}" for c in (launch(case, prob, frames, rep) or [])]
        complaints += [f"rep {rep}: {c}" for c in frame_damage(case, frames)]
        for p, f in zip(prob, frames):
            got.append(view_c(case, f).reshape(-1))
            ref.append(p["ref"].reshape(-1))
            mag.append(p["mag"].reshape(-1))
    got, ref, mag = torch.cat(got), torch.cat(ref), torch.cat(mag)
    g = gate_of(case)
    worst, exact = stats(got, ref, mag, g["ulps"])
    print(f"{case.id}: {got.numel()} outputs, worst err/tol {worst:.3f}, bit-exact {exact:.5f}")
    assert not complaints, f"{case.id}: " + "; ".join(complaints[:6])
    assert_close_mag(got, ref, mag=mag, what=case.id, **g)
    return worst, exact
