"""Column edges and K stages: the GEMM kernels have more column- and K-dependent paths than row-dependent ones — the 16-byte / 8-byte
store choice of the 16-bit epilogues (N % 8, ldo % 8), the row-per-lane epilogue's per-8-column mask behind two permlane32_swaps, the
32-column staging rounds of the OVL epilogue, whole waves or parts of a wave outside a 256-column tile (N % 256), W rows clamped at
N - 1 for the DMA, the guarded float4 bias load, the persistent loop's wait path after a partial column tile, and on the K side the
one- / odd- / even-stage pipelines, the ring of three, and gemm.hip's register-staged ragged K tail.  test_row_edges_gpu.py sweeps M at
N = 768, K = 256 — whole tiles and an even stage count — and the other GEMM tests know column residues 4 and 8 and one ragged K only.
These tests sweep N and K through s3enc_op_gemm, score every COLUMN on its own against float64 (one wrong column in 380 moves a
Frobenius norm very little), check NaN-prefilled guard rows (behind every batch) and guard columns, and — because N changes no product
and no summation order — demand that a call with N columns equals, bit for bit, the leading N columns of the same call at N = 512.

The 16-bit families' fp32 output is held to the fp32 band (the reference sees the operands the kernel sees, accumulation is fp32)."""

import dataclasses
import functools
import math
import zlib

import numpy as np
import pytest

from test_ops_gpu import TOL, _dev, _ptr, _round, _torch
from test_row_edges_gpu import EPI16, EPI32, FAMILIES, GUARD, _limit, _set, assert_guards, guarded

pytestmark = pytest.mark.gpu

N_MAX = 512  # columns of every operand set; a call with N columns uses the leading N rows of W
M_ROWS = 161  # one 192- / 256-row tile, two 128-row tiles, a partial 32-row block (161 % 32 = 1)
FLOOR = 1e-3
# out32 of these families meets the fp32 band: exact 16-bit products, fp32 accumulation, the reference built from the same operands
SHARP = ("bf16", "fp16", "fp16x2")


def _epis(family):
    """name -> (act, residual, row_limit, out32, out16) of the family's epilogue instantiations (swish: the exact-fp32 kernels only)."""
    code = FAMILIES[family][0]
    epis = EPI32 if code in (0, 3) else EPI16
    return {k: v[:5] for k, v in epis.items() if not (code == 3 and v[0] == 3)}


# ---- operands and the float64 reference, once per (family, shape) -------------------------------------------------------------------
class _Run:
    """Device operands of one (family, K, M, batches, lda, a_bs) and the float64 pre-activation product on the device."""

    def __init__(self, family, K, M, batches, lda, a_bs, n_max=N_MAX, hi_only=False):
        torch = _torch()
        from s3prl_amd import _lib

        self.lib = _lib.load()
        self.check = _lib.check
        self.family, self.K, self.M, self.batches, self.lda, self.a_bs, self.n_max = family, K, M, batches, lda, a_bs, n_max
        self.code, rnd, self.tk = FAMILIES[family][:3]
        self.t16 = torch.bfloat16 if rnd == "bf16" else torch.float16
        rng = np.random.default_rng(zlib.crc32(f"col_edges/{family}/{K}/{M}/{batches}/{lda}/{a_bs}/{n_max}".encode()))
        A = _round(rng.standard_normal((batches, a_bs)).astype(np.float32), rnd)
        W = (rng.standard_normal((n_max, K)) / np.sqrt(K)).astype(np.float32)
        bias = rng.standard_normal(n_max).astype(np.float32)
        res = rng.standard_normal((batches, M, n_max)).astype(np.float32)
        if self.code == 4:  # [hi | lo] fp16 halves per row: the product is with hi + lo (K % 64 != 0: with hi alone, s3enc.h)
            Wt = torch.from_numpy(W)
            hi = Wt.half()
            lo = (Wt - hi.float()).half()
            self.W = torch.cat([hi, lo], dim=1).contiguous().cuda()
            W64 = hi.double().numpy() + (0 if hi_only else lo.double().numpy())
        elif self.code in (1, 2):
            self.W, W64 = _dev(W, rnd), _round(W, rnd).astype(np.float64)
        else:  # fp32 / fp32x3 / the MX entry take the fp32 weight (the latter two pack it inside the call)
            self.W, W64 = _dev(W), W.astype(np.float64)
        self.A, self.bias = _dev(A, rnd), _dev(bias)
        idx = (np.arange(M) * lda)[:, None] + np.arange(K)[None, :]  # row m of a batch starts at m * lda (lda < K: conv windows)
        lin = A.astype(np.float64)[:, idx] @ W64.T + bias
        self.lin = torch.from_numpy(lin).cuda()
        self.res32 = torch.from_numpy(res).cuda()
        self.res64 = self.res32.double()
        lim = np.array([_limit(M) if b % 2 == 0 else M - 5 - b % 7 for b in range(batches)], dtype=np.int32)
        self.lim = torch.from_numpy(lim).cuda()
        self.limmask = (torch.arange(M, device="cuda")[None, :] >= self.lim[:, None].long())[:, :, None]
        self._res, self._ref = (None, None), (None, None)

    def residual(self, B, N, ldo):
        """The residual re-laid at the call's ldo and batch stride (M + GUARD rows per batch), NaN wherever the call must not read."""
        torch = _torch()
        if self._res[0] != (B, N, ldo):
            r = torch.full((B, self.M + GUARD, ldo), float("nan"), device="cuda")
            r[:, :self.M, :N] = self.res32[:B, :, :N]
            self._res = ((B, N, ldo), r)
        return self._res[1]

    def reference(self, B, N, epi):
        """(ref, per-column norm floored, whole norm, 1 + |ref|) of the epilogue of lin[..., :N], float64 on the device."""
        torch = _torch()
        act, use_res, use_lim = epi[:3]
        if self._ref[0] != (B, N, act, use_res, use_lim):
            y = self.lin[:B, :, :N]
            if act == 1:
                y = 0.5 * y * (1.0 + torch.erf(y * (1.0 / math.sqrt(2.0))))
            elif act == 3:
                y = y * torch.sigmoid(y)
            if use_res:
                y = y + self.res64[:B, :, :N]
            if use_lim:
                y = y.masked_fill(self.limmask[:B], 0.0)
            y = y.contiguous()
            self._ref = ((B, N, act, use_res, use_lim),
                         (y, y.pow(2).sum(dim=(0, 1)).sqrt().clamp_min(FLOOR), y.norm().clamp_min(1e-30), 1.0 + y.abs()))
        return self._ref[1]

    def launch(self, N, ldo, epi, what, batches=None):
        """One s3enc_op_gemm with N columns; returns the NaN-prefilled (batches, M + GUARD, ldo) buffers (out32, out16)."""
        torch = _torch()
        act, use_res, use_lim, o32, o16 = epi
        B, M = batches or self.batches, self.M
        rows = B * (M + GUARD) - GUARD
        b32 = guarded(rows, N, torch.float32, ldo)[0].view(B, M + GUARD, ldo) if o32 else None
        b16 = guarded(rows, N, self.t16, ldo)[0].view(B, M + GUARD, ldo) if o16 else None
        rc = self.lib.s3enc_op_gemm(self.code, _ptr(self.A), self.lda, self.a_bs, _ptr(self.W), _ptr(self.bias), M, N, self.K, B, act,
                                    _ptr(self.residual(B, N, ldo)) if use_res else None, _ptr(self.lim) if use_lim else None,
                                    _ptr(b32), _ptr(b16), ldo, (M + GUARD) * ldo, None)
        self.check(rc, what)
        return b32, b16


@functools.lru_cache(maxsize=2)
def _run(family, K, M, batches, lda, a_bs, n_max=N_MAX, hi_only=False):
    return _Run(family, K, M, batches, lda, a_bs, n_max, hi_only)


# ---- scoring: everything on the device, one host copy per group of launches -----------------------------------------------------
@dataclasses.dataclass
class _Rec:
    what: str
    out: str
    buf: object
    M: int
    N: int
    tol_all: float
    tol_col: float
    tol_elem: float
    peers: list  # names of what `stats` compared bit for bit
    stats: object


class _Scorer:
    def __init__(self, family):
        self.family = family
        self.tol = TOL[FAMILIES[family][2]]
        self.pending, self.fails, self.worst = [], [], {}

    def add(self, run, buf, out, N, epi, what, peers=(), score=True, batches=None):
        """Queue the checks of one output buffer: guards, finiteness, (score) the float64 bands per column, bit-identity with
        every (name, buffer) of `peers` over their common leading columns."""
        torch = _torch()
        M = run.M
        v = buf[:, :M, :N]
        z = torch.zeros((), device="cuda", dtype=torch.float64)
        st = [(~torch.isfinite(v)).sum(), (~torch.isnan(buf[:, M:, :])).sum(), (~torch.isnan(buf[:, :M, N:])).sum()]
        if score:
            ref, col_den, tot_den, absr1 = run.reference(batches or run.batches, N, epi)
            d = v.double() - ref
            csq = (d * d).sum(dim=(0, 1))
            w, wi = (csq.sqrt() / col_den).max(dim=0)
            st += [csq.sum().sqrt() / tot_den, w, wi, (d.abs() > (50 * self.tol) * absr1).sum() if out == "out32" else z]
        else:
            st += [z, z, z, z]
        for _, other in list(peers) + [(None, None)] * (2 - len(peers)):
            if other is None:
                st += [z, z]
            else:
                nec = (v != other[:, :M, :N]).sum(dim=(0, 1))
                st += [nec.sum(), (nec > 0).to(torch.int8).argmax()]
        sharp = out == "out32" and self.family in SHARP
        tol = TOL["fp32"] if sharp else self.tol
        if out == "out32":
            bounds = (tol, 2 * tol, 50 * self.tol)
        else:
            bounds = (2 * self.tol, 4 * self.tol, 0.0)  # (test_gemm's whole-tensor band of the 16-bit output)
        if not score:
            bounds = (math.inf, math.inf, 0.0)
        self.pending.append(_Rec(what, out, buf, M, N, *bounds, [n for n, _ in peers], torch.stack([x.double() for x in st])))

    def flush(self):
        torch = _torch()
        if not self.pending:
            return
        S = torch.stack([r.stats for r in self.pending]).cpu().numpy()
        for r, s in zip(self.pending, S):
            nonfin, hit_rows, hit_cols, rel, w, wi, bad = s[:7]
            what, N, n = f"{r.what} {r.out}", r.N, int(wi)
            col = f"column {n} of N = {N} (n % 8 = {n % 8}, n % 32 = {n % 32}, n % 64 = {n % 64}, N % 256 = {N % 256})"
            if hit_rows or hit_cols:
                try:
                    for b in range(r.buf.shape[0]):
                        assert_guards(r.buf[b], r.M, N, f"{what} batch {b}")
                except AssertionError as e:
                    self.fails.append(str(e))
            if nonfin:
                self.fails.append(f"{what}: {int(nonfin)} non-finite values inside the product")
                continue
            if not rel < r.tol_all:
                self.fails.append(f"{what}: rel-err {rel:.3e} >= {r.tol_all:.1e}")
            if not w < r.tol_col:
                self.fails.append(f"{what}: worst {col}: per-column error {w:.3e} >= {r.tol_col:.1e}")
            if bad:
                self.fails.append(f"{what}: {int(bad)} elements off by more than {r.tol_elem:.1e} (1 + |ref|)")
            for i, name in enumerate(r.peers):
                neq, n = s[7 + 2 * i], int(s[8 + 2 * i])
                if neq:
                    self.fails.append(f"{what}: {int(neq)} elements differ from {name}, first in column {n} of N = {N} "
                                      f"(n % 8 = {n % 8}, n % 32 = {n % 32}, n % 64 = {n % 64}, N % 256 = {N % 256})")
            if math.isfinite(r.tol_col) and w > self.worst.get(r.out, (-1.0,))[0]:
                self.worst[r.out] = (float(w), f"{what}: {col}", float(rel))
        self.pending.clear()

    def finish(self, title):
        self.flush()
        for out, (w, where, rel) in sorted(self.worst.items()):
            print(f"COLEDGE {title} {out}: worst per-column error {w:.3e} (rel-err of that launch {rel:.3e}) at {where}")
        assert not self.fails, (f"{title}: {len(self.fails)} failed checks, the first {min(len(self.fails), 12)}:\n  " +
                                "\n  ".join(self.fails[:12]))


def _mode_name(key, mode):
    return "" if key is None else f" {key} = {mode}"


def _sweep(sc, run, N, ldo, name, epi, key, modes, title, bases=None, batches=None):
    """One (N, ldo, epilogue) in every mode of `key`: scoring 1-3 per launch, fp32: every mode bit-identical to the first (4),
    `bases`: mode -> (out32, out16) of the same call at N_MAX, bit-identical over the leading N columns (5)."""
    first = None
    for mode in modes:
        if key is not None:
            _set(run.lib, key, mode)
        what = f"{title} N = {N} K = {run.K} ldo = {ldo} {name}{_mode_name(key, mode)}"
        b32, b16 = run.launch(N, ldo, epi, what, batches)
        for out, buf, i in (("out32", b32, 0), ("out16", b16, 1)):
            if buf is None:
                continue
            peers = []
            if bases is not None:
                peers.append((f"the same call at N = {N_MAX}", bases[mode][i]))
            if key == "gemm32_big":  # (gemm_variant's 64- and 128-byte stages sum k in different orders: no such identity)
                if first is None:
                    first = buf
                else:
                    peers.append((f"{key} = {modes[0]}", first))
            sc.add(run, buf, out, N, epi, what, peers, batches=batches)
    sc.flush()


# ---- part A: every column residue ---------------------------------------------------------------------------------------------------
A_NS = list(range(128, 384, 4))  # every multiple-of-4 residue mod 256 once, every residue mod 128 twice


def _a_cases():
    cases = []
    for family in FAMILIES:
        names = list(_epis(family))
        # ldo = N + 64: guard columns.  ldo = N: the engine's own layout, an over-wide store lands in the next row.  ldo = N + 36:
        # ldo % 8 == 4 forces the 8-byte store path at N % 8 == 0 and takes the row-per-lane epilogue away from modes 9 and 10
        cases += [(family, n, 64) for n in names]
        cases += [(family, n, x) for n in ("out16", "act_out16", "res_out32") if n in names for x in (0, 36)]
    return cases


@pytest.mark.parametrize("family,name,extra", _a_cases(), ids=lambda v: f"ldo+{v}" if isinstance(v, int) else v)
def test_gemm_at_every_column_residue(family, name, extra):
    """M = 161, batches = 2, K = 192 (fp16x2_mx: 256), N = 128, 132 ... 380 in every kernel mode of the family: scoring 1-5.  The
    N = 512 baseline of check 5 is taken in the same mode: with M = 161 and two batches big_mode / launch_gemm_x3 pick the 192-row tile
    for every N <= 512, and the shape-chosen tile heights of gemmt.hip (gemm32_big / gemm_x3_tile = 1) are bit-identical to each other."""
    K = 256 if family == "fp16x2_mx" else 192
    run = _run(family, K, M_ROWS, 2, K, M_ROWS * K)
    key, modes, default = FAMILIES[family][3:]
    epi = _epis(family)[name]
    sc = _Scorer(family)
    title = f"{family} A"
    try:
        bases = {}
        for mode in modes:
            if key is not None:
                _set(run.lib, key, mode)
            bases[mode] = run.launch(N_MAX, N_MAX + extra, epi, f"{title} N = {N_MAX} {name}{_mode_name(key, mode)}")
        for N in A_NS:
            _sweep(sc, run, N, N + extra, name, epi, key, modes, title, bases)
    finally:
        if key is not None:
            _set(run.lib, key, default)
    sc.finish(f"{title} {name} ldo = N + {extra}")


# ---- part B: narrow and non-multiple-of-4 N -----------------------------------------------------------------------------------------
B_NS = [1, 2, 3, 4, 5, 7, 8, 31, 33, 63, 64, 65, 100, 124, 127, 129, 130, 131, 258]


@pytest.mark.parametrize("family", ["fp32", "bf16", "fp16", "fp16x2"])
def test_gemm_at_narrow_and_unaligned_columns(family):
    """gemm.hip's 128x128 kernel with its scalar epilogue (N or ldo = N + 3 is never a multiple of 4 together): every staging
    variant, 35 = variant 3 with the scalar epilogue forced.  Scoring 1-3."""
    K = 192
    run = _run(family, K, M_ROWS, 2, K, M_ROWS * K)
    sc = _Scorer(family)
    epis = _epis(family)
    try:
        for N in B_NS:
            for name in ("row_limit", "res_out32"):
                _sweep(sc, run, N, N + 3, name, epis[name], "gemm_variant", (0, 1, 2, 3, 35), f"{family} B")
    finally:
        _set(run.lib, "gemm_variant", 3)
    sc.finish(f"{family} B")


# ---- part C: every K-stage count and K tail --------------------------------------------------------------------------------------
C_NS = (132, 380)
C_KS = {
    "bf16": range(64, 513, 64), "fp16": range(64, 513, 64), "fp16x2": range(64, 513, 64),  # 1..8 stages of 64 k (mode 4: 2..16 of 32)
    "fp16x2_mx": range(128, 513, 128), "fp32": range(16, 161, 16), "fp32x3": range(32, 257, 32),
}


def _c_run(family, K, hi_only=False):
    lda = K + 16  # a kernel that strides by K instead of lda, or batches by M * lda, reads the wrong rows
    return _run(family, K, M_ROWS, 2, lda, M_ROWS * lda + 32, N_MAX, hi_only)


@pytest.mark.parametrize("family", list(C_KS))
def test_gemm_at_every_k_stage_count(family):
    """K through every stage count of the pipelines (one stage: nothing to overlap; odd: ends on the other buffer; the ring of
    three), lda = K + 16, in every mode (fp16x2: every gemm16_big mode too).  Scoring 1-4."""
    key, modes, default = FAMILIES[family][3:]
    if family == "fp16x2":
        key, modes, default = FAMILIES["fp16"][3:]
    epis = _epis(family)
    sc = _Scorer(family)
    lib = None
    try:
        for K in C_KS[family]:
            run = _c_run(family, K)
            lib = run.lib
            for N in C_NS:
                for name in ("row_limit", "res_out32"):
                    _sweep(sc, run, N, N + 64, name, epis[name], key, modes, f"{family} C")
    finally:
        if key is not None and lib is not None:
            _set(lib, key, default)
    sc.finish(f"{family} C")


@pytest.mark.parametrize("family", ["fp32", "bf16", "fp16", "fp16x2"])
def test_gemm_at_every_ragged_k_tail(family):
    """K = 1..17 granules of 16 bytes through gemm.hip (the tile kernels switched off: they take whole stages only) in every staging
    variant: every tail of a 64-byte and of a 128-byte stage behind zero, one and two whole stages.  fp16x2 at K % 64 != 0 is the
    product with the hi half alone (s3enc.h).  Scoring 1-3."""
    big, big_default = ("gemm32_big", 1) if family == "fp32" else ("gemm16_big", 3)
    epis = _epis(family)
    sc = _Scorer(family)
    lib = None
    try:
        for g in range(1, 18):
            K = (4 if family == "fp32" else 8) * g
            run = _c_run(family, K, hi_only=family == "fp16x2" and K % 64 != 0)
            lib = run.lib
            _set(lib, big, 0)
            for N in C_NS:
                for name in ("row_limit", "res_out32"):
                    _sweep(sc, run, N, N + 64, name, epis[name], "gemm_variant", (0, 1, 2, 3), f"{family} ragged K ({g} granules)")
    finally:
        if lib is not None:
            _set(lib, big, big_default)
            _set(lib, "gemm_variant", 3)
    sc.finish(f"{family} ragged K")


@pytest.mark.parametrize("family", ["fp32", "bf16", "fp16"])
def test_gemm_on_narrow_conv_windows(family):
    """conv1-4 of a narrow extractor: Conv1d(C, C, k = 3, s = 2) on channel-last rows, N = C, K = 3C, lda = 2C < K, GELU — K = 96,
    288, 480, 672 are 1.5, 4.5 ... stages of 64 k.  Scoring 1-3."""
    M = M_ROWS
    Lin = 2 * M + 1
    sc = _Scorer(family)
    names = ("act_out32",) if family == "fp32" else ("act_out16", "act_out32")
    epis = _epis(family)
    lib = None
    try:
        for Cc in (32, 96, 160, 224):
            run = _run(family, 3 * Cc, M, 2, 2 * Cc, Lin * Cc, Cc)
            lib = run.lib
            for name in names:
                _sweep(sc, run, Cc, Cc, name, epis[name], "gemm_variant", (0, 1, 2, 3), f"{family} conv C = {Cc}")
    finally:
        if lib is not None:
            _set(lib, "gemm_variant", 3)
    sc.finish(f"{family} conv windows")


# ---- part D: partial column tiles inside the persistent tile walk ---------------------------------------------------------------
D_NS = (132, 252, 260, 316, 324, 380,
        136, 376)  # N % 8 == 0: the only ones at which modes 9 / 10 (and 7 under GELU) take the row-per-lane epilogue inside the walk
D_TILES = 160
D_RESERVE = 128


@pytest.mark.parametrize("family,K", [("bf16", 64), ("bf16", 192), ("fp16", 64), ("fp16", 192), ("fp16x2_mx", 128), ("fp16x2_mx", 256)])
def test_partial_column_tiles_inside_the_persistent_walk(family, K):
    """160 tiles of 192 x 256 on CUs - 128 persistent workgroups: some workgroups walk two tiles, and at these N every second (or
    every) tile is partial in its columns — the persistent loop then cannot count the previous tile's stores and takes its other
    wait path.  Modes 7-10 on the small grid are bit-identical to the one-shot grid of mode 1 (MX: to reserve_cus = 0), which is
    scored (1-3) and compared with its own N = 512 run at the same batches (5).  N = 136 and 376 add the row-per-lane epilogue, which
    needs N % 8 == 0, to the walk."""
    torch = _torch()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus - D_RESERVE < D_TILES <= cus, f"{cus} CUs: {D_TILES} tiles do not make a {cus - D_RESERVE}-workgroup grid walk"
    run = _run(family, K, M_ROWS, D_TILES, K, M_ROWS * K)
    lib = run.lib
    mx = family == "fp16x2_mx"
    epis = _epis(family)
    sc = _Scorer(family)
    title = f"{family} D"
    try:
        for name in ("act_out16", "out16", "res_out32", "row_limit"):
            epi = epis[name]
            bases = {}
            for N in D_NS:
                B = D_TILES // ((N + 255) // 256)
                _set(lib, "reserve_cus", 0)
                if not mx:
                    _set(lib, "gemm16_big", 1)
                if B not in bases:
                    bases[B] = run.launch(N_MAX, N_MAX + 64, epi, f"{title} N = {N_MAX} {name} batches = {B}", B)
                what = f"{title} N = {N} K = {K} batches = {B} {name}"
                one = run.launch(N, N + 64, epi, what + " one-shot grid", B)
                for out, buf, base in zip(("out32", "out16"), one, bases[B]):
                    if buf is not None:
                        sc.add(run, buf, out, N, epi, what + " one-shot grid", [(f"the same call at N = {N_MAX}", base)], batches=B)
                _set(lib, "reserve_cus", D_RESERVE)
                for mode in (7,) if mx else (7, 8, 9, 10):
                    if not mx:
                        _set(lib, "gemm16_big", mode)
                    w = what + (f" reserve_cus = {D_RESERVE}" if mx else f" gemm16_big = {mode} reserve_cus = {D_RESERVE}")
                    walk = run.launch(N, N + 64, epi, w, B)
                    for out, buf, ref in zip(("out32", "out16"), walk, one):
                        if buf is not None:
                            sc.add(run, buf, out, N, epi, w, [("the one-shot grid", ref)], score=False, batches=B)
                sc.flush()
    finally:
        _set(lib, "reserve_cus", 0)
        _set(lib, "gemm16_big", 3)
    sc.finish(f"{title} K = {K}")
