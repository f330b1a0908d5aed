"""CPU-side checks of the real-valued Input's C ABI (include/snnhip.h f17): the three entry points are declared, exported and bound,
they refuse null pointers and zero sizes before touching a GPU, snn_layer_desc's float twins sit where the ctypes mirror puts them,
and snn_net_run's validation refuses what a real-valued Input may not drive.  No compute calls here."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("snn_prop_dense_real_f32", "snn_prop_conv2d_real_f32", "snn_input_step_real_pv")
INVALID, UNSUPPORTED = -1, -2


def test_new_symbols_are_declared_exported_and_bound():
    from bindsnet_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "snnhip.h")).read()
    declared = set(re.findall(r"\b(snn_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for sym in NEW:
        assert sym in declared and sym in _lib.exported_symbols() and hasattr(L, sym), sym
    assert "-ffp-contract=off" in hdr and "f17" in hdr
    for fn in ("prop_dense_real", "prop_conv2d_real", "input_step_real"):
        assert callable(getattr(ops, fn))
    assert L.snn_abi_version() == _lib.ABI_VERSION == 8          # additive: the version stays


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from bindsnet_amd import _lib
    L = _lib.lib()
    d = L.snn_prop_dense_real_f32
    assert d(None, None, 1, 1, 1, 1, 1, 0, None) == INVALID and d(1, None, None, 1, 1, 1, 1, 0, None) == INVALID
    assert d(1, None, 1, None, 1, 1, 1, 0, None) == INVALID
    for B, Nin, N in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)):
        assert d(1, None, 1, 1, B, Nin, N, 0, None) == INVALID
    assert d(1, None, 1, 1, 1, 1 << 24, 1, 0, None) == UNSUPPORTED and d(1, None, 1, 1, 65536, 1, 1, 0, None) == UNSUPPORTED
    c = L.snn_prop_conv2d_real_f32
    ok = dict(B=1, Cin=1, H=5, Wd=5, Cout=1, KH=3, KW=3, stride=1, pad=0)
    assert c(None, None, 1, 1, *ok.values(), 0, None) == INVALID and c(1, None, None, 1, *ok.values(), 0, None) == INVALID
    assert c(1, None, 1, None, *ok.values(), 0, None) == INVALID
    for key, bad in (("B", 0), ("Cin", 0), ("H", 0), ("Wd", 0), ("Cout", 0), ("KH", 0), ("KW", 0), ("stride", 0), ("pad", -1), ("KH", 6), ("KW", 6)):
        assert c(1, None, 1, 1, *dict(ok, **{key: bad}).values(), 0, None) == INVALID, (key, bad)
    # the int limits of snn_prop_conv2d_f32: taps, image, output plane
    assert c(1, None, 1, 1, *dict(ok, Cin=1 << 20, KH=50, KW=50, H=50, Wd=50).values(), 0, None) == UNSUPPORTED
    assert c(1, None, 1, 1, *dict(ok, H=1 << 16, Wd=1 << 16, KH=1, KW=1).values(), 0, None) == UNSUPPORTED
    s = L.snn_input_step_real_pv
    assert s(None, 1, 1, 1, 0.5, 1.0, 0, None, None, None) == INVALID
    assert s(1, 1, 0, 1, 0.5, 1.0, 0, None, None, None) == INVALID and s(1, 1, 1, 0, 0.5, 1.0, 0, None, None, None) == INVALID
    assert s(1, 1, 65536, 1, 0.5, 1.0, 0, None, None, None) == UNSUPPORTED
    pv = _lib.PerVec()
    pv.v[_lib.PERVEC.index("trace_scale")] = 1
    assert s(1, 1, 1, 1, 0.5, 1.0, 0, C.byref(pv), None, None) == INVALID          # a per-neuron trace_scale needs additive traces
    pv = _lib.PerVec()
    pv.v[_lib.PERVEC.index("thresh")] = 1
    assert s(1, 1, 1, 1, 0.5, 1.0, 1, C.byref(pv), None, None) == INVALID          # a vector an Input does not read
    assert s(1, None, 1, 1, 0.5, 1.0, 0, None, None, None) == 0                    # neither trace nor raster: nothing to launch


def test_layer_descriptor_twins_match_the_header():
    from bindsnet_amd import _lib
    fields = ("summed", "ext_real", "s_real", "raster_real")
    src = '#include "snnhip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(){printf("%zu ' + "%zu " * len(fields) + '\\n",sizeof(snn_layer_desc),' \
          + ",".join(f"offsetof(snn_layer_desc,{f})" for f in fields) + ");return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [C.sizeof(_lib.LayerDesc)] + [getattr(_lib.LayerDesc, f).offset for f in fields]
    assert [n for n, _ in _lib.LayerDesc._fields_][-3:] == list(fields[1:])


def _graph(conn_kind, real=True, rule=0, dst_kind=None, **conn):
    """Input(4) -> conn -> LIF(4) with dummy pointers: only snn_net_run's validation may look at them."""
    from bindsnet_amd import _lib
    L = (_lib.LayerDesc * 2)()
    L[0].kind, L[0].n = _lib.LAYER_INPUT, 4
    if real:
        L[0].ext_real, L[0].s_real = 64, 64
    else:
        L[0].ext_spikes, L[0].s = 64, 64
    L[1].kind, L[1].n = _lib.LAYER_LIF if dst_kind is None else dst_kind, 4
    L[1].v = L[1].refrac = L[1].s = L[1].current = L[1].x = 64
    Cn = (_lib.ConnDesc * 1)()
    Cn[0].kind, Cn[0].src, Cn[0].dst, Cn[0].w, Cn[0].rule, Cn[0].wdecay = conn_kind, 0, 1, 64, rule, 1.0
    for k, v in conn.items():
        setattr(Cn[0], k, v)
    R = _lib.RunDesc()
    R.B, R.T, R.dt = 1, 1, 1.0
    return L, Cn, R


def test_net_run_validation_of_a_real_valued_input():
    from bindsnet_amd import _lib
    lib = _lib.lib()

    def run(L, Cn, R):
        return lib.snn_net_run(L, 2, Cn, 1, C.byref(R), None)

    # every connection kind but DENSE and CONV2D out of a real-valued Input
    assert run(*_graph(_lib.CONN_MCC)) == UNSUPPORTED
    assert run(*_graph(_lib.CONN_LOCAL, local_src=64, cin=1, local_F=1, local_conv_prod=4, local_kernel_prod=1, local_n_src=4)) == UNSUPPORTED
    assert run(*_graph(_lib.CONN_CONVND, conv_nd=1, cin=1, conv_d=1, h=1, wd=4, cout=1, conv_kd=1, kh=1, kw=1)) == UNSUPPORTED
    assert run(*_graph(_lib.CONN_SPARSE, w=None, sparse_ptr=64)) == UNSUPPORTED
    assert run(*_graph(_lib.CONN_MEANFIELD, w_numel=1)) == UNSUPPORTED
    assert run(*_graph(_lib.CONN_PERMUTE, w=None)) == UNSUPPORTED and run(*_graph(_lib.CONN_PAD, w=None)) == UNSUPPORTED
    assert run(*_graph(_lib.CONN_POOL, w=None, firing_rates=64, pool_c=1)) == UNSUPPORTED
    # a learning rule on such a connection
    for rule in (_lib.RULE_POSTPRE, _lib.RULE_HEBBIAN, _lib.RULE_MSTDP):
        assert run(*_graph(_lib.CONN_DENSE, rule=rule, p_plus=64, p_minus=64, s_src_prev=64, s_tgt_prev=64)) == UNSUPPORTED
        assert run(*_graph(_lib.CONN_CONV2D, rule=rule, rule_ws=64, cin=1, h=2, wd=2, cout=1, kh=1, kw=1, stride=1)) == UNSUPPORTED
    # a windowed (CSRM) target
    L, Cn, R = _graph(_lib.CONN_DENSE, dst_kind=_lib.LAYER_CSRM, window=1, win_ring=64, win_size=2)
    L[1].csrm_xwin = L[1].csrm_last = L[1].csrm_resk = L[1].csrm_refk = L[1].theta = 64
    L[1].csrm_wres = L[1].csrm_wref = 2
    assert run(L, Cn, R) == UNSUPPORTED
    # the twins belong to a real-valued INPUT layer alone
    L, Cn, R = _graph(_lib.CONN_DENSE)
    L[0].s = 64
    assert run(L, Cn, R) == INVALID
    L, Cn, R = _graph(_lib.CONN_DENSE)
    L[0].s_real = None
    assert run(L, Cn, R) == INVALID
    L, Cn, R = _graph(_lib.CONN_DENSE, real=False)
    L[0].raster_real = 64
    assert run(L, Cn, R) == INVALID
    L, Cn, R = _graph(_lib.CONN_DENSE, real=False)
    L[1].ext_real = 64
    assert run(L, Cn, R) == INVALID
