"""The original per-operator kernels of csrc/snn_ops.hip across their launch limits, on the MI355X, against the CPU oracle bit for bit.

Every entry point is called through bindsnet_amd.ops at the shapes of tests/ops_sweep_cases.py, whose rows name the limit they
straddle; tests/test_ops_sweep_host.py pins the oracle at the same shapes against torch on the CPU first.  Outputs are NaN-prefilled
where the op stores, the accumulate variant runs where the op has one, and every tensor an op writes sits in front of guard elements
that must come back untouched.

  * normalize (k_colsum / k_colsum_few / k_scale_cols): row counts on either side of the 16-row block, of the folds at 16 and 256
    blocks and of the 64-block round, every Nin % 4 with order-dependent weights, column counts with no tail, only a tail, one tail
    column, one column and four to seven columns (ATen's own rules for those: an inner reduction, the first four on the cascade),
    the second grid pass of k_scale_cols; both `use_abs`; a zeroed column.
  * propagation (k_prop / k_prop_col1): N and Nin around the 256-column workgroup, the 256-entry wave list and the 1024-source
    chunk, a spike in the last slot, every list full, spike bytes 1 / 2 / 255; prop_cascade, prop_dense with and without bias.
  * narrow conv2d (k_conv2d): a request of 69 120 B of dynamic LDS (beyond 64 KiB: the launcher sets
    hipFuncAttributeMaxDynamicSharedMemorySize) and a control below, images too large to stage (nstage == 0), a block that spans
    more samples than the batch has left, KH != KW, multi-valued spike bytes.
  * Input / LIF steps (k_input, k_lif, k_lif<VTH>, k_lif_pv): exactly the grid cap and one element past it, both trace kinds, both
    rasters, neurons that spike, sit out the refractory period and rest on lbound.
  * Diehl&Cook step (k_dc_membrane, k_dc_arbitrate): N around the wave and the 256-thread stride, B on several ranking rounds;
    steps in which every row, no row, only row 0 and only row B - 1 cross; one_spike off; hand-built ties in one wave, two waves,
    one thread's two strides and across the fold, the winner the lowest index in each.
  * scalar plasticity (k_plasticity<TJ>): B on either side of every tile threshold of launch_plasticity AT THIS COMMIT (TJ = 256 up
    to B = 46, 128 up to 88, 64 up to 159, 32 up to 256; ops_sweep_cases.plasticity_tile restates the formula and the host test
    asserts the table), N = 2 TJ + 3 and TJ, Nin = 15, 17, 33 (kTI = 16): PostPre with and without dt, Hebbian,
    WeightDependentPostPre, MSTDP with a scalar reward and a reward vector; assume_clamped; B = 257 refused with W unchanged.
  * grid caps of k_mstdp_traces (B (Nin + N) > 2048 x 256) and k_mstdpet (Nin N > 4096 x 256)."""
import numpy as np
import pytest
import torch

import oracle
import ops_sweep_cases as SC
import test_ops_sweep_host as H
from test_gpu_ops import DEV, bits, dev, host, lifp

pytestmark = pytest.mark.gpu
f32, u8 = np.float32, np.uint8
GUARD = 7


def guarded(a):
    """A device copy of the numpy array `a` with 4096 guard elements behind it, and the guard: a write past the end shows there."""
    a = np.ascontiguousarray(a)
    src = torch.from_numpy(a)
    buf = torch.full((a.size + 4096,), GUARD, dtype=src.dtype, device=DEV)
    t = buf[:a.size].view(a.shape)
    t.copy_(src)
    return t, buf[a.size:]


def intact(*guards):
    return all(bool((g == GUARD).all()) for g in guards)


def same(got, want):
    got = host(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == f32:
        got, want = bits(got), bits(want)
    return np.array_equal(got, want)


def nans(shape):
    return guarded(np.full(shape, np.nan, f32))


# ---------------------------------------------------------------------------------------------------------------- normalize
@pytest.mark.parametrize("use_abs", [False, True])
@pytest.mark.parametrize("Nin,N,zero", H.normalize_cases())
def test_normalize(Nin, N, zero, use_abs):
    from bindsnet_amd import ops
    W0, want = H.run_normalize_oracle(Nin, N, use_abs, zero)          # (asserts the zero column kept and another one changed)
    Wd, g = guarded(W0)
    ops.normalize(Wd, SC.NORM, use_abs)
    got = host(Wd)
    assert np.array_equal(bits(got), bits(want)), (Nin, N, use_abs, int((bits(got) != bits(want)).sum()))
    assert intact(g)


# ---------------------------------------------------------------------------------------------------------------- propagation
@pytest.mark.parametrize("B,Nin,N", SC.prop_shapes())
def test_propagation(B, Nin, N):
    from bindsnet_amd import ops
    W, bias, prev, patterns = SC.prop_inputs(B, Nin, N)
    Wd, bd = dev(W), dev(bias)
    for name, s in patterns:
        sd = dev(s)
        for label, fn, ref, b in (("cascade", ops.prop_cascade, oracle.prop_mcc, None), ("dense", ops.prop_dense, oracle.prop_dense, None),
                                  ("dense+bias", ops.prop_dense, oracle.prop_dense, bias)):
            kw = {} if label == "cascade" else dict(bias=None if b is None else bd)
            rkw = {} if label == "cascade" else dict(bias=b)
            out, g = nans((B, N))
            fn(Wd, sd, out, **kw)
            assert same(out, ref(W, s, **rkw)), (label, name)
            acc, ga = guarded(prev)
            fn(Wd, sd, acc, accumulate=True, **kw)
            assert same(acc, ref(W, s, out=prev.copy(), accumulate=True, **rkw)), (label, name, "accumulate")
            assert intact(g, ga)


# ---------------------------------------------------------------------------------------------------------------- narrow conv2d
@pytest.mark.parametrize("row", SC.CONV_ROWS, ids=lambda r: f"b{r[0]}_cin{r[1]}_{r[2]}x{r[3]}_cout{r[4]}_k{r[5][0]}x{r[5][1]}_s{r[6]}p{r[7]}_v{len(r[8])}")
def test_narrow_conv2d(row):
    from bindsnet_amd import ops
    B, Cin, Hh, Wd_, Cout, (KH, KW), stride, pad, values = row
    W, bias, spikes = SC.conv_inputs(row)
    Wd, bd = dev(W), dev(bias)
    rng = SC.rng_of(37, B, Cout)
    for density, s in spikes:
        want = oracle.prop_conv2d(W, s, bias=bias, stride=stride, pad=pad)
        prev = rng.standard_normal(want.shape).astype(f32)
        sd = dev(s)
        out, g = nans(want.shape)
        ops.prop_conv2d(Wd, sd, out, bias=bd, stride=stride, pad=pad)
        assert same(out, want), (row, density, int((bits(host(out)) != bits(want)).sum()))
        acc, ga = guarded(prev)
        ops.prop_conv2d(Wd, sd, acc, bias=None, stride=stride, pad=pad, accumulate=True)
        assert same(acc, prev + oracle.prop_conv2d(W, s, stride=stride, pad=pad)), (row, density, "accumulate")
        assert intact(g, ga)
        assert len(values) == 1 or (s == 255).any()


# ---------------------------------------------------------------------------------------------------------------- Input / LIF
def _lif_params(kind, **kw):
    k = SC.LIF_KW
    return lifp(decay=k["decay"], rest=k["rest"], reset=k["reset"], thresh=k["thresh"], refrac=k["refrac0"], has_lbound=1, lbound=k["lbound"],
                traces=1, trace_decay=kind["trace_decay"], trace_scale=kind["trace_scale"], traces_additive=int(kind["additive"]), **kw)


def _lif_on_device(I, kind, ref, **step_kw):
    from bindsnet_amd import ops
    T, B, N = I.shape
    state = [guarded(a) for a in (np.full((B, N), SC.LIF_KW["rest"], f32), np.zeros((B, N), f32), np.full((B, N), 9, u8), np.zeros((B, N), f32))]
    (v, gv), (r, gr), (s, gs), (x, gx) = state
    (Id, gI), (ras_s, g1), (ras_v, g2) = guarded(I), guarded(np.full((T, B, N), 9, u8)), nans((T, B, N))
    p = _lif_params(kind)
    for t in range(T):
        ops.lif_step(v, r, s, x, Id[t], p, raster_s=ras_s[t], raster_v=ras_v[t], **step_kw)
    for got, key in ((v, "v"), (r, "r"), (s, "s"), (x, "x"), (Id, "I"), (ras_s, "ras_s"), (ras_v, "ras_v")):
        assert same(got, ref[key]), key
    assert intact(gv, gr, gs, gx, gI, g1, g2)


@pytest.mark.parametrize("kind", [0, 1], ids=["set", "additive"])
@pytest.mark.parametrize("B,N", SC.LIF_SHAPES)
def test_lif_step(B, N, kind):
    kind = SC.TRACE_KINDS[kind]
    I = SC.lif_currents(B, N)
    ref = H.run_lif_oracle(I, kind)
    assert H.lif_is_active(ref) == (B * N >= 255)               # (one neuron cannot spike AND reach lbound in six steps: the host test's docstring)
    _lif_on_device(I, kind, ref)


@pytest.mark.parametrize("form", ["thresh_vec", "pv"])
def test_lif_step_with_per_neuron_thresholds(form):
    """thresh_vec alone takes k_lif<VTH> (k % N), the same vector as a per-neuron parameter takes k_lif_pv."""
    B, N = 3, 257
    I, th, kind = SC.lif_currents(B, N), SC.lif_thresholds(N), SC.TRACE_KINDS[0]
    ref = H.run_lif_oracle(I, kind, th)
    assert H.lif_is_active(ref)
    _lif_on_device(I, kind, ref, **(dict(thresh_vec=dev(th)) if form == "thresh_vec" else dict(pv=dict(thresh=dev(th)))))


@pytest.mark.parametrize("kind", [0, 1], ids=["set", "additive"])
@pytest.mark.parametrize("B,N", SC.INPUT_SHAPES)
def test_input_step(B, N, kind):
    from bindsnet_amd import ops
    kind = SC.TRACE_KINDS[kind]
    sp = SC.input_spikes(B, N)
    want = H.run_input_oracle(sp, kind)
    (x, gx), (ras, gr) = guarded(np.zeros((B, N), f32)), guarded(np.full(sp.shape, 9, u8))
    spd = dev(sp)
    for t in range(sp.shape[0]):
        ops.input_step(spd[t], x, kind["trace_decay"], kind["trace_scale"], kind["additive"], raster=ras[t])
    assert same(x, want) and same(ras, sp) and intact(gx, gr)
    assert sp.any() == (B * N > 1)


# ---------------------------------------------------------------------------------------------------------------- Diehl&Cook
def _dc_params(one_spike=True):
    from bindsnet_amd._lib import DcParams
    k = SC.DC_KW
    p = DcParams()
    p.lif = lifp(decay=k["decay"], rest=k["rest"], reset=k["reset"], thresh=k["thresh"], refrac=k["refrac0"], traces=1, trace_decay=k["trace_decay"])
    p.theta_decay, p.theta_plus, p.learning, p.one_spike = k["theta_decay"], k["theta_plus"], 1, int(one_spike)
    return p


def _dc_on_device(I, Q, ref, one_spike=True):
    from bindsnet_amd import ops
    T, B, N = I.shape
    (v, gv), (r, gr), (s, gs), (x, gx) = (guarded(a) for a in (np.full((B, N), SC.DC_KW["rest"], f32), np.zeros((B, N), f32),
                                                                np.full((B, N), 9, u8), np.zeros((B, N), f32)))
    (theta, gt), (ras, g1), (ras_v, g2) = guarded(np.zeros(N, f32)), guarded(np.full((T, B, N), 9, u8)), nans((T, B, N))
    cursor, status = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    Id, Qd, p = dev(I), dev(Q), _dc_params(one_spike)
    consumed = []
    for t in range(T):
        ops.dc_step(v, r, s, x, theta, Id[t], p, Qd, cursor, status, raster_s=ras[t], raster_v=ras_v[t])
        consumed.append(int(cursor[0].item()))
    assert int(status.item()) == 0
    assert consumed == [int(c) * N for c in np.cumsum(ref["rows"])] and consumed[-1] == ref["cursor"]
    for got, key in ((v, "v"), (r, "r"), (s, "s"), (x, "x"), (theta, "theta"), (ras, "ras")):
        assert same(got, ref[key]), key
    assert same(ras_v[-1], ref["v"]) and intact(gv, gr, gs, gx, gt, g1, g2)


@pytest.mark.parametrize("B,N", SC.dc_shapes())
def test_dc_step(B, N):
    I, Q = SC.dc_inputs(B, N)
    ref = H.run_dc_oracle(I, Q)
    H.check_dc_rows(B, N, ref)
    _dc_on_device(I, Q, ref)
    _dc_on_device(I, Q, H.run_dc_oracle(I, Q, one_spike=False), one_spike=False)


@pytest.mark.parametrize("lo,hi,what", SC.DC_TIES, ids=[f"{t[0]}_{t[1]}" for t in SC.DC_TIES])
def test_dc_ties_go_to_the_lowest_index(lo, hi, what):
    from bindsnet_amd import ops
    I, Q = SC.dc_tie_inputs(lo, hi)
    B, N = I.shape
    ref = H.run_dc_oracle(I[None], Q)
    assert [row.nonzero()[0].tolist() for row in ref["s"]] == [[lo]] * B            # the oracle's answer (pinned to torch.argmax on the host)
    _dc_on_device(I[None], Q, ref)
    # the arbitration alone, on the same crossings
    (s, gs), (x, gx), (ras, g1) = guarded((I > 0).astype(u8)), guarded(np.zeros((B, N), f32)), guarded(np.full((B, N), 9, u8))
    cursor, status = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.dc_arbitrate(s, x, _dc_params(), dev(Q), cursor, status, raster_s=ras)
    assert same(s, ref["s"]) and same(ras, ref["s"]) and same(x, ref["x"]), what
    assert cursor.tolist() == [B * N, 0] and int(status.item()) == 0 and intact(gs, gx, g1)


# ---------------------------------------------------------------------------------------------------------------- plasticity
def _apply_rule(rule, Wd, arrays, B, decay=SC.WDECAY, **kw):
    from bindsnet_amd import ops
    s_src, x_src, s_tgt, x_tgt = (dev(a) for a in arrays)
    nu0, nu1 = H.plasticity_rates(rule, B)
    if rule.startswith("postpre"):
        ops.stdp_postpre(Wd, s_src, x_src, s_tgt, x_tgt, nu0, nu1, use_dt=rule == "postpre_dt", dt=0.5, decay=decay, wmin=SC.WMIN, wmax=SC.WMAX, **kw)
    else:
        ops.stdp_hebbian(Wd, s_src, x_src, s_tgt, x_tgt, nu0, nu1, weight_dependent=rule == "wdpp", decay=decay, wmin=SC.WMIN, wmax=SC.WMAX)


def _mstdp_on_device(W, s_src, s_tgt, reward, reward_vec, want):
    from bindsnet_amd import ops
    T, B, Nin = s_src.shape
    N = s_tgt.shape[2]
    Ws, pp, pm = want
    k = SC.MSTDP_KW
    (Wd, gw), (ppd, g1), (pmd, g2) = guarded(W), guarded(np.zeros((B, Nin), f32)), guarded(np.zeros((B, N), f32))
    (sp, g3), (tp, g4) = guarded(np.zeros((B, Nin), u8)), guarded(np.zeros((B, N), u8))
    rv = None if reward_vec is None else dev(reward_vec)
    for t in range(T):
        ops.mstdp_step(Wd, ppd, pmd, sp, tp, dev(s_src[t]), dev(s_tgt[t]), reward, k["nu0"], k["a_plus"], k["a_minus"], k["decay_plus"],
                       k["decay_minus"], wdecay=SC.WDECAY, wmin=SC.WMIN, wmax=SC.WMAX, reward_vec=rv)
        assert same(Wd, Ws[t]), (t, int((bits(host(Wd)) != bits(Ws[t])).sum()))
    assert same(ppd, pp) and same(pmd, pm) and same(sp, s_src[-1]) and same(tp, s_tgt[-1]) and intact(gw, g1, g2, g3, g4)


@pytest.mark.parametrize("B", sorted(SC.PLASTICITY_B))
def test_scalar_plasticity_tiles(B):
    """All constants are plain floats: k_plasticity<TJ>, not k_plasticity_pv."""
    for shape in SC.plasticity_shapes(B):
        W0, *arrays = SC.plasticity_inputs(*shape)
        quiet = [np.zeros_like(arrays[0]), arrays[1], np.zeros_like(arrays[2]), arrays[3]]
        for rule in H.PLASTICITY_RULES:
            want = H.run_plasticity_oracle(rule, W0, *arrays)
            H.check_bounds_and_motion(W0, want, H.run_plasticity_oracle(rule, W0, *quiet))
            for kw in ([{}, dict(assume_clamped=True)] if rule.startswith("postpre") else [{}]):      # (decay != 1: the flag must change nothing)
                Wd, g = guarded(W0)
                _apply_rule(rule, Wd, arrays, B, **kw)
                assert same(Wd, want), (shape, rule, kw, int((bits(host(Wd)) != bits(want)).sum()))
                assert intact(g)
        # assume_clamped where it skips: decay 1, weights inside the bounds, silent rows, columns and tiles
        Wi, *sparse = SC.plasticity_inputs(*shape, inside=True, sparse=True)
        for rule in ("postpre_dt", "postpre"):
            want = H.run_plasticity_oracle(rule, Wi, *sparse, decay=1.0)
            assert (want != Wi).any() and (want == Wi).any()
            for clamped in (False, True):
                Wd, g = guarded(Wi)
                _apply_rule(rule, Wd, sparse, B, decay=1.0, assume_clamped=clamped)
                assert same(Wd, want) and intact(g), (shape, rule, clamped)
        W, s_src, s_tgt, rv = SC.mstdp_inputs(*shape)
        for reward, vec in ((0.7, None), (0.0, rv)):
            _mstdp_on_device(W, s_src, s_tgt, reward, vec, H.run_mstdp_oracle(W, s_src, s_tgt, reward, vec))


def test_plasticity_refuses_more_than_256_samples():
    """B = 257: SNN_ERR_UNSUPPORTED (-2) from every scalar entry point, raised by ops before anything is launched; W as it was."""
    from bindsnet_amd import _lib, ops
    B, Nin, N = 257, 17, 35
    W0, s_src, x_src, s_tgt, x_tgt = SC.plasticity_inputs(B, Nin, N)
    Wd, g = guarded(W0)
    a = [dev(t) for t in (s_src, x_src, s_tgt, x_tgt)]
    with pytest.raises(_lib.SnnError, match=r"code -2"):
        ops.stdp_postpre(Wd, *a, 1e-3, 1e-3, use_dt=True, wmin=SC.WMIN, wmax=SC.WMAX)
    with pytest.raises(_lib.SnnError, match=r"code -2"):
        ops.stdp_hebbian(Wd, *a, 1e-3, 1e-3, wmin=SC.WMIN, wmax=SC.WMAX)
    with pytest.raises(_lib.SnnError, match=r"code -2"):
        ops.stdp_hebbian(Wd, *a, 1e-3, 1e-3, weight_dependent=True, wmin=SC.WMIN, wmax=SC.WMAX)
    pp, pm = dev(x_src), dev(x_tgt)
    with pytest.raises(_lib.SnnError, match=r"code -2"):
        ops.mstdp_step(Wd, pp, pm, dev(s_src), dev(s_tgt), dev(s_src), dev(s_tgt), 0.5, 1e-2, 1.0, -1.0, 0.9, 0.9, wmin=SC.WMIN, wmax=SC.WMAX)
    assert same(Wd, W0) and same(pp, x_src) and same(pm, x_tgt) and intact(g)


def test_mstdp_traces_beyond_the_grid_cap():
    B, Nin, N = SC.MSTDP_CAP
    W, s_src, s_tgt, rv = SC.mstdp_inputs(B, Nin, N)
    _mstdp_on_device(W, s_src, s_tgt, 0.7, None, H.run_mstdp_oracle(W, s_src, s_tgt, 0.7))


def test_mstdpet_beyond_the_grid_cap():
    from bindsnet_amd import ops
    Nin, N = SC.MSTDPET_CAP
    W, s_src, s_tgt, _ = SC.mstdp_inputs(1, Nin, N)
    s_src, s_tgt = s_src[:, 0], s_tgt[:, 0]
    steps, pp, pm = H.run_mstdpet_oracle(W, s_src, s_tgt)
    k = H.MSTDPET_KW
    (Wd, gw), (et, ge), (ppd, g1), (pmd, g2) = guarded(W), guarded(np.zeros((Nin, N), f32)), guarded(np.zeros(Nin, f32)), guarded(np.zeros(N, f32))
    (sp, g3), (tp, g4) = guarded(np.zeros(Nin, u8)), guarded(np.zeros(N, u8))
    for t in range(SC.MSTDP_STEPS):
        ops.mstdpet_step(Wd, et, ppd, pmd, sp, tp, dev(s_src[t]), dev(s_tgt[t]), k["reward"], k["nu0"], k["dt"], k["a_plus"], k["a_minus"],
                         k["decay_plus"], k["decay_minus"], k["decay_e"], k["tc_e"], wdecay=SC.WDECAY, wmin=SC.WMIN, wmax=SC.WMAX)
        assert same(Wd, steps[t][0]) and same(et, steps[t][1]), t
    assert same(ppd, pp) and same(pmd, pm) and same(sp, s_src[-1]) and same(tp, s_tgt[-1]) and intact(gw, ge, g1, g2, g3, g4)
    H.check_mstdpet_activity(W, steps)


# ---------------------------------------------------------------------------------------------------------------- the fused plans
@pytest.mark.parametrize("kind,N", [("mcc", 4), ("mcc", 5), ("mcc", 7), ("dense", 6)])
def test_fused_two_layer_plan_follows_the_few_column_order(kind, N):
    """Four to seven target neurons: the fused plan's propagation (MCC) and its closing normalisation (both kinds) put the first four
    columns on the cascade like the generic plan, which the rows above pin to the oracle and so to torch."""
    from test_gpu_fuzz import _same, two
    f, plan = two.run(False, kind, 256, N, 7, 12, True, False, dens=0.2)
    g, plan_g = two.run(True, kind, 256, N, 7, 12, True, False, dens=0.2)
    assert (plan, plan_g) == ("twolayer-fused", "generic")
    _same(f, g, f"twolayer {kind} N={N}")


def test_fused_plans_leave_the_smallest_layers_to_the_generic_plan():
    """One target neuron (an inner reduction) in the two-layer graph, fewer than eight in the Diehl&Cook graph: no fused plan offers itself."""
    import synth
    from test_gpu_fuzz import dc, two
    _, plan = two.run(False, "mcc", 256, 1, 3, 8, True, False, dens=0.2)
    assert plan == "generic"
    spikes = [synth.dense_spikes(900 + r, (8, 2, 784), 0.05) for r in range(2)]
    _, plan = dc.run(0, 5, 2, 8, spikes)
    assert plan == "generic"
