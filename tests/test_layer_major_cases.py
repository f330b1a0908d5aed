"""The table of tests/layer_major_cases.py on the host: every case still has the geometry it is named for (the kernel's formulas
restated in Python), and the float64 reference of every newer case fires neither never nor always, so that an equal train says something."""
import pytest
import torch

from layer_major_cases import CASES, EVERY_LAYER, NEW, STAGE_WORDS, band_of, geometry, byte2_frames, khw, padded_terms, references, slab_count, spike_share, wide_pixel_stride


def test_the_restatements_on_figures_worked_by_hand():
    assert [wide_pixel_stride(c) for c in (1, 16, 17, 32, 33, 49, 64, 97)] == [16, 16, 48, 48, 48, 80, 80, 112]
    assert padded_terms(49, 7, 7) == 3136 and slab_count(49, 7, 7) == 49 and slab_count(97, 5, 5) == 44 and slab_count(17, 1, 3) == 2
    g = geometry(CASES["stage_overflow"][0])
    assert [band_of(p0, g) for p0 in (0, 64, 128)] == [(0, 4), (1, 6), (4, 4)] and g["words"] == [1920, 2880, 1920] and STAGE_WORDS == 2048
    g = geometry(CASES["pad_beyond_half"][0])                       # 49 output pixels in one block: all five input rows
    assert band_of(0, g) == (0, 5) and g["words"] == [5 * 5 * 12]
    g = geometry(CASES["stride2"][0])
    assert (g["OH"], g["OW"], g["blocks"], g["packed"]) == (5, 4, 1, True)
    g = geometry(CASES["byte2_traces"][0], 1)                       # the second conv reads the first one's output
    assert (g["Cin"], g["H"], g["W"], g["nps"], g["packed"]) == (20, 9, 7, 63, False)


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][4] is not None])
def test_a_case_reaches_the_branch_it_is_named_for(name):
    assert CASES[name][4](geometry(CASES[name][0])), geometry(CASES[name][0])


def test_the_restated_residency_is_the_library_s():
    """snn_run_conv2d_sif_takes is a fact of the shape and touches no device: 0 refused, 1 resident, 2 streaming.  (It is asked of
    the built library, like every host test that loads it: build first.)"""
    from bindsnet_amd import ops
    for name, (spec, T, B, opt, _) in CASES.items():
        (cin, H, W), (_, cout, k, stride, pad) = spec[0], spec[1][0]
        want = 0 if name == "refused_bytes" else 1 if geometry(spec)["resident"] else 2
        assert ops.run_conv2d_sif_takes(T, B, cin, H, W, cout, *khw(k), stride, pad) == want, name


@pytest.mark.parametrize("name", NEW)
def test_the_reference_fires_some_of_the_time(name):
    for trains, _ in references(name)[2]:
        assert 0.05 <= spike_share(trains) <= 0.95, [spike_share([t]) for t in trains]


@pytest.mark.parametrize("name", EVERY_LAYER)
def test_every_layer_of_the_reference_fires_some_of_the_time(name):
    for trains, _ in references(name)[2]:
        assert all(0.05 <= spike_share([t]) <= 0.95 for t in trains), [spike_share([t]) for t in trains]


@pytest.mark.parametrize("name", list(CASES))
def test_a_byte_above_one_sits_in_the_frame_the_case_names(name):
    """stream_odd_byte2: input frame 1 of run 0 feeds step 2, so the steps are matrix, matrix, scalar, matrix, matrix;
    stream_odd_byte2_run2: frame 0 of run 1 feeds that run's step 1.  No other case or frame holds a byte above 1."""
    T, opt = CASES[name][1], CASES[name][3]
    assert byte2_frames(name) == ([] if opt.get("analog") else [(r, min(f, T - 1)) for r, f in opt.get("two", ())])
    assert name not in ("stream_odd_byte2", "stream_odd_byte2_run2") or T == 5


def test_traces_of_the_reference():
    """Set and additive traces differ on one train (so that no single body passes both operator variants), and the chain with traces
    holds traces that are neither all 0 nor all 1."""
    x, s = torch.tensor([0.25, 0.25]).double(), torch.tensor([0.0, 1.0]).double()
    from layer_major_cases import trace_next
    assert trace_next(x, s, 0.5, 1.0, False).tolist() == [0.125, 1.0] and trace_next(x, s, 0.5, 1.0, True).tolist() == [0.125, 1.125]
    for _, state in references("byte2_traces_sparse")[2]:
        for xk in state["x"]:
            assert len(set(xk.flatten().tolist())) >= 4
