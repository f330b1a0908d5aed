"""The float16 / bfloat16 kernels' arithmetic on the HOST: tests/hostcheck/half_host.hip compiles the __host__ __device__ bodies of
csrc/snn_half.hpp with hipcc (no GPU needed) and drives them as the kernels of csrc/snn_half.hip do.

  * the conversion helpers against tensor.to(dtype): every one of the 65 536 patterns widened and narrowed back, and a float sweep with
    ties, subnormals, overflow to +-inf and NaN.  A NaN is compared as a NaN: which payload a conversion keeps is the converter's
    business (torch's own scalar and vector paths differ), and no weight is one;
  * propagation, PostPre and normalisation against the reference's torch statements (half_cases.ref_*), raw bits, over
    N in {1, 7, 33, 40, 400} x Nin in {17, 100, 784} x B in {1, 3, 33} (33 crosses batch_sum's 32-term classes) x density in
    {0, 0.02, 0.3, 1} x accumulate, the rule variants of half_cases.RULES, a zero column and norm 78.4."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import half_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CODES = {torch.float16: 1, torch.bfloat16: 2}
DTYPES = sorted(CODES, key=CODES.get)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    out = str(tmp_path_factory.mktemp("hostcheck") / "libhalfhost.so")
    src = os.path.join(ROOT, "tests", "hostcheck", "half_host.hip")
    subprocess.run([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out],
                   check=True, capture_output=True, timeout=600)
    lib = C.CDLL(out)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    lib.hostcheck_half_widen.argtypes = lib.hostcheck_half_narrow.argtypes = [vp, vp, C.c_long, i]
    lib.hostcheck_half_prop.argtypes = [vp, i, vp, vp, i, i, i, i]
    lib.hostcheck_half_postpre.argtypes = [vp, i, vp, vp, vp, vp, i, i, i, f, f, i, f, f, i, f, i, f]
    lib.hostcheck_half_normalize.argtypes = [vp, i, i, i, f, vp]
    return lib


def _p(t):
    return C.c_void_p(t.data_ptr())


class HostImpl:
    """The three operations on CPU tensors through the host bodies (tests/test_gpu_half.py has the same interface over ops.*)."""

    def __init__(self, lib):
        self.lib = lib

    def prop(self, W, s, out, accumulate):
        B, (Nin, N) = s.shape[0], W.shape
        assert self.lib.hostcheck_half_prop(_p(W), CODES[W.dtype], _p(s), _p(out), B, Nin, N, int(accumulate)) == 0
        return out

    def postpre(self, W, s_src, x_src, s_tgt, x_tgt, nu0, nu1, dt, decay, lo, hi):
        B, (Nin, N) = s_src.shape[0], W.shape
        assert self.lib.hostcheck_half_postpre(_p(W), CODES[W.dtype], _p(s_src), _p(x_src), _p(s_tgt), _p(x_tgt), B, Nin, N, nu0, nu1, 1, dt,
                                               decay, int(lo is not None), lo or 0.0, int(hi is not None), hi or 0.0) == 0
        return W

    def normalize(self, W, norm):
        Nin, N = W.shape
        factor = torch.empty(N)                                  # (the column workspace: alive across the call)
        assert self.lib.hostcheck_half_normalize(_p(W), CODES[W.dtype], Nin, N, norm, _p(factor)) == 0
        return W


def same_bits(got, want, what):
    if got.dtype == torch.float32:
        g, w = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    else:
        g, w = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    bad = int((g != w).sum())
    assert bad == 0, f"{what}: {bad} of {g.numel()} elements differ"


# ---- the sweeps, shared with the device test --------------------------------------------------------------------------------------
def sweep_prop(impl, dtype, N, to=lambda t: t):
    rng = np.random.default_rng(100 + N + CODES[dtype])
    for Nin in HC.SWEEP_NIN:
        W = HC.rand_weights(rng, Nin, N, dtype, scale=1.0) - 0.25       # both signs
        for B in HC.SWEEP_B:
            for density in HC.SWEEP_DENSITY:
                s = HC.rand_spikes(rng, B, Nin, density)
                before = torch.from_numpy(rng.standard_normal((B, N)).astype(np.float32))
                for acc in (False, True):
                    out = to(before.clone()) if acc else to(torch.full((B, N), float("nan")))
                    got = impl.prop(to(W), to(s), out, acc).cpu()
                    same_bits(got, HC.ref_prop(W, s, before if acc else None), f"prop {dtype} N={N} Nin={Nin} B={B} density={density} acc={acc}")


def sweep_postpre(impl, dtype, B, to=lambda t: t):
    rng = np.random.default_rng(200 + B + CODES[dtype])
    changed = {rule: 0 for rule in HC.RULES}
    for N in HC.SWEEP_N:
        for Nin in HC.SWEEP_NIN:
            W0 = HC.rand_weights(rng, Nin, N, dtype, scale=0.4)
            s_src, s_tgt = HC.rand_spikes(rng, B, Nin, 0.3), HC.rand_spikes(rng, B, N, 0.3)
            x_src = torch.from_numpy(rng.random((B, Nin)).astype(np.float32))
            x_tgt = torch.from_numpy(rng.random((B, N)).astype(np.float32))
            for rule, (nu0, nu1, decay, (lo, hi), dt) in HC.RULES.items():
                want, f0, f1, factor = HC.ref_postpre(W0, s_src, x_src, s_tgt, x_tgt, nu0, nu1, decay, lo, hi, dt)
                got = impl.postpre(to(W0.clone()), to(s_src), to(x_src), to(s_tgt), to(x_tgt), f0, f1, dt, factor, lo, hi).cpu()
                same_bits(got, want, f"postpre {dtype} rule={rule} N={N} Nin={Nin} B={B}")
                changed[rule] += int((got.view(torch.int16) != W0.view(torch.int16)).sum())
    assert min(changed.values()) > 0, f"a rule variant changed no weight in the whole sweep: {changed}"


def sweep_normalize(impl, dtype, to=lambda t: t):
    rng = np.random.default_rng(300 + CODES[dtype])
    for N in HC.SWEEP_N:
        for Nin in HC.SWEEP_NIN:
            for norm in (78.4, 1.0):
                W = HC.rand_weights(rng, Nin, N, dtype, scale=0.3)
                W[:, N // 2] = 0                                        # a zero column: its sum is replaced by 1
                if N > 2:
                    W[:, 1] = -W[:, 1]                                  # a negative column sum (the sums are signed)
                same_bits(impl.normalize(to(W.clone()), norm).cpu(), HC.ref_normalize(W, norm), f"normalize {dtype} N={N} Nin={Nin} norm={norm}")


# ---- conversions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_65536_patterns_widen_and_narrow_back(host, dtype):
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)        # every 16-bit pattern (wraps to the signed range)
    want = pat.view(dtype).float()
    wide = torch.empty(65536)
    assert host.hostcheck_half_widen(_p(pat), _p(wide), 65536, CODES[dtype]) == 0
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(wide), nan) and int(nan.sum()) > 0
    same_bits(wide[~nan], want[~nan], f"{dtype}: widened patterns")
    back = torch.empty(65536, dtype=torch.int16)
    assert host.hostcheck_half_narrow(_p(wide), _p(back), 65536, CODES[dtype]) == 0
    assert torch.equal(back[~nan], pat[~nan]), f"{dtype}: narrowing a widened pattern does not give it back"
    assert torch.isnan(back.view(dtype)[nan].float()).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_narrowing_rounds_like_torch(host, dtype):
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).float()
    fin = pat[torch.isfinite(pat)].view(torch.int32)
    step = 1 << (13 if dtype == torch.float16 else 16)                  # the float32 bits below the narrow format's last place
    # around every representable value: itself, the tie above it, and both neighbours of that tie
    sweep = torch.cat([fin, fin + step // 2, fin + step // 2 - 1, fin + step // 2 + 1, fin + 1, fin + step - 1])
    rng = np.random.default_rng(7)
    extra = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32),      # any pattern, NaNs among them
                            np.float32([65504.0, 65519.9, 65520.0, 65536.0, 1e30, 3.3895e38, 3.4e38, np.inf, -np.inf, np.nan, 0.0, -0.0,
                                        5.96e-8, 2.98e-8, 2.9802322e-8, 2.99e-8, 1e-40, 1e-45, -1e-40, 6.1e-5, 6.0975552e-5])])
    x = torch.cat([sweep.view(torch.float32), torch.from_numpy(extra), -torch.from_numpy(extra)]).contiguous()
    want = x.to(dtype)
    got = torch.empty(x.numel(), dtype=torch.int16)
    assert host.hostcheck_half_narrow(_p(x), _p(got), x.numel(), CODES[dtype]) == 0
    nan = torch.isnan(x)
    assert int(nan.sum()) > 0 and torch.isnan(got.view(dtype)[nan].float()).all()
    same_bits(got.view(dtype)[~nan], want[~nan], f"{dtype}: float32 -> {dtype}")
    assert torch.isinf(want[~nan].float()).sum() > torch.isinf(x[~nan]).sum(), "no finite value of the sweep overflows"


# ---- the three bodies -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", HC.SWEEP_N)
@pytest.mark.parametrize("dtype", DTYPES)
def test_propagation_body_equals_torch(host, dtype, N):
    sweep_prop(HostImpl(host), dtype, N)


@pytest.mark.parametrize("B", HC.SWEEP_B)
@pytest.mark.parametrize("dtype", DTYPES)
def test_postpre_body_equals_torch(host, dtype, B):
    sweep_postpre(HostImpl(host), dtype, B)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_one_sum_reduction_equals_the_squeeze(dtype):
    """DiehlAndCook2015 makes its rule before its layers have a batch size, so its reduction is torch.sum at batch 1 too: for the
    non-negative traces and rates of a network both give the bits the kernel's batch-1 path is checked against."""
    rng = np.random.default_rng(5)
    W0 = HC.rand_weights(rng, 100, 33, dtype)
    s_src, s_tgt = HC.rand_spikes(rng, 1, 100, 0.3), HC.rand_spikes(rng, 1, 33, 0.3)
    x_src, x_tgt = torch.from_numpy(rng.random((1, 100)).astype(np.float32)), torch.from_numpy(rng.random((1, 33)).astype(np.float32))
    a = HC.ref_postpre(W0, s_src, x_src, s_tgt, x_tgt, 1e-2, 5e-2, 0.01, 0.1, 0.3, 0.5, reduction=torch.sum)[0]
    b = HC.ref_postpre(W0, s_src, x_src, s_tgt, x_tgt, 1e-2, 5e-2, 0.01, 0.1, 0.3, 0.5, reduction=torch.squeeze)[0]
    same_bits(a, b, "sum over one sample against squeeze")


@pytest.mark.parametrize("dtype", DTYPES)
def test_normalize_body_equals_torch(host, dtype):
    sweep_normalize(HostImpl(host), dtype)


def test_an_inhibition_sum_beyond_float16_overflows_to_minus_infinity_like_torch(host):
    """400 spiking sources at -200 each: -80 000 is beyond float16's 65 504.  The reference's half sum is -inf, and so is the body's."""
    W = torch.full((400, 7), -200.0, dtype=torch.float16)
    s = torch.ones(2, 400, dtype=torch.uint8)
    want = HC.ref_prop(W, s)
    assert torch.isinf(want).all() and (want < 0).all()
    same_bits(HostImpl(host).prop(W, s, torch.zeros(2, 7), False), want, "overflowing inhibition")
    same_bits(HostImpl(host).prop(W.to(torch.bfloat16), s, torch.zeros(2, 7), False), HC.ref_prop(W.to(torch.bfloat16), s), "the same in bfloat16: finite")
