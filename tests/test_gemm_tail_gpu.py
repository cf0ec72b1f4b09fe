"""Mixed-height launches of the exact-fp32 tile GEMM (gemmt.hip, tuning key gemm32_tail) are bit-identical to gemm.hip's kernel.

A launch of 128 / 192 / 256-row tiles may end with a tail region of 64-row tiles run by the same kernel.  Every height sums
each accumulator in the same k order on the same instruction, so whatever the bulk / tail split — chosen by shape (1) or forced
to the largest tail (2) — every output bit must equal gemm32_big = 0, for every epilogue the kernel has: plain, bias + GELU,
bias + residual into a separate buffer and in place (out == residual, the residual vectors are requested ahead of the stores),
and row_limit below M."""

import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

M_VALUES = (64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 383, 385, 449)  # every residue around a bulk / tail /
N_VALUES = (128, 132, 256)                                                             # ragged-last-tile boundary of 128, 192, 256
K_VALUES = (16, 32, 48, 768)  # one, two, three K steps (the pipeline prologue and its odd tail) and the path's K
EPILOGUES = ("plain", "bias_gelu", "bias_residual", "bias_residual_inplace", "row_limit")
VARIANTS = [(tail, big) for tail in (1, 2) for big in (1, 2, 3, 4)]


def _torch():
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _gemm(lib, _lib, A, W, bias, M, N, K, nb, act, res, lim, out):
    _lib.check(lib.s3enc_op_gemm(0, _ptr(A), K, M * K, _ptr(W), _ptr(bias), M, N, K, nb, act, _ptr(res), _ptr(lim), _ptr(out), None,
                                 N, M * N, None))


def _run_case(torch, lib, _lib, epilogue, A, W, bias, res, M, N, K, nb):
    """One shape and epilogue: the reference under gemm32_big = 0, then every (gemm32_tail, gemm32_big) variant against it."""
    use_bias = epilogue != "plain"
    act = 1 if epilogue == "bias_gelu" else 0
    use_res = epilogue in ("bias_residual", "bias_residual_inplace")
    inplace = epilogue == "bias_residual_inplace"
    lim = torch.tensor([M - 7 * (b + 1) for b in range(nb)], dtype=torch.int32, device="cuda") if epilogue == "row_limit" else None
    b_ = bias if use_bias else None
    r_ = res[: nb * M * N] if use_res else None
    _lib.check(lib.s3enc_set_tuning(b"gemm32_big", 0))
    ref = torch.full((nb * M * N,), float("nan"), device="cuda")
    _gemm(lib, _lib, A, W, b_, M, N, K, nb, act, r_, lim, ref)  # the in-place variants must equal the two-buffer result
    bad = []
    for tail, big in VARIANTS:
        _lib.check(lib.s3enc_set_tuning(b"gemm32_tail", tail))
        _lib.check(lib.s3enc_set_tuning(b"gemm32_big", big))
        if inplace:
            out = r_.clone()
            _gemm(lib, _lib, A, W, b_, M, N, K, nb, act, out, lim, out)
        else:
            out = torch.full((nb * M * N,), float("nan"), device="cuda")
            _gemm(lib, _lib, A, W, b_, M, N, K, nb, act, r_, lim, out)
        if not torch.equal(ref, out):
            bad.append((tail, big, int((ref != out).sum())))
    assert bool(torch.isfinite(ref).all()), "the reference left elements unwritten"
    return bad


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("epilogue", EPILOGUES)
def test_tail_launches_are_bit_identical_to_the_128x128_kernel(epilogue, nb):
    torch = _torch()
    from s3prl_amd import _lib

    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(1234 + 17 * nb + EPILOGUES.index(epilogue))
    Mx, Nx, Kx = max(M_VALUES), max(N_VALUES), max(K_VALUES)
    A_all = torch.randn(nb * Mx * Kx, device="cuda", generator=g)
    W_all = torch.randn(Nx * Kx, device="cuda", generator=g)
    bias = torch.randn(Nx, device="cuda", generator=g)
    res = torch.randn(nb * Mx * Nx, device="cuda", generator=g)
    failures = []
    try:
        for K in K_VALUES:
            for N in N_VALUES:
                W = W_all[: N * K] / K ** 0.5
                for M in M_VALUES:
                    bad = _run_case(torch, lib, _lib, epilogue, A_all[: nb * M * K], W, bias[:N], res, M, N, K, nb)
                    failures += [(M, N, K) + b for b in bad]
    finally:
        _lib.check(lib.s3enc_set_tuning(b"gemm32_big", 1))
        _lib.check(lib.s3enc_set_tuning(b"gemm32_tail", 1))
    assert not failures, f"(M, N, K, gemm32_tail, gemm32_big, differing values): {failures[:20]} ({len(failures)} in all)"


def test_shape_chosen_tail_on_a_launch_of_more_than_one_round():
    """M = 131072 + 192, N = 128, K = 16: 1026 tiles of 128 rows (513 of 256) — one whole round of a 256-CU part and a remainder,
    which gemm32_tail = 1 turns into a tail of three 64-row tiles; the automatic path, not only the forced one."""
    torch = _torch()
    from s3prl_amd import _lib

    lib = _lib.load()
    M, N, K = 131072 + 192, 128, 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus == 256:
        for tm in (2, 4):
            n0, n1 = C.c_int64(0), C.c_int64(0)
            _lib.check(lib.s3enc_debug_gemm_schedule(M, N, 1, tm, 0, cus, None, 0, C.byref(n0)))
            _lib.check(lib.s3enc_debug_gemm_schedule(M, N, 1, tm, 1, cus, None, 0, C.byref(n1)))
            assert n1.value == n0.value + tm // 2, f"tm = {tm}: the shape rule chose no tail ({n0.value} -> {n1.value} workgroups)"
    g = torch.Generator(device="cuda").manual_seed(99)
    A = torch.randn(M * K, device="cuda", generator=g)
    W = torch.randn(N * K, device="cuda", generator=g) / K ** 0.5
    bias = torch.randn(N, device="cuda", generator=g)
    res = torch.randn(M * N, device="cuda", generator=g)
    try:
        bad = _run_case(torch, lib, _lib, "bias_residual_inplace", A, W, bias, res, M, N, K, 1)
        bad += _run_case(torch, lib, _lib, "bias_gelu", A, W, bias, res, M, N, K, 1)
    finally:
        _lib.check(lib.s3enc_set_tuning(b"gemm32_big", 1))
        _lib.check(lib.s3enc_set_tuning(b"gemm32_tail", 1))
    assert not bad, f"(gemm32_tail, gemm32_big, differing values): {bad}"
