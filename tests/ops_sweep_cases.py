"""Shapes and seeded inputs of the per-operator launch-limit sweep (csrc/snn_ops.hip): plain data, shared by
tests/test_ops_sweep_host.py (the oracle against torch on the CPU) and tests/test_gpu_ops_sweep.py (the device against the oracle).
Every row names the limit of its kernel that it straddles; every builder draws from numpy's default_rng with a seed made of the
row, so both files see the same numbers."""
import itertools

import numpy as np

f32, u8 = np.float32, np.uint8


def rng_of(*key):
    """default_rng seeded by the integers of a row (no hash(): the same stream in every process)."""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (1 << 63)
    return np.random.default_rng(seed)


def thin(product, step, factors):
    """Every `step`-th combination; each value of each factor must survive."""
    kept = list(product)[::step]
    for axis, values in enumerate(factors):
        assert {s[axis] for s in kept} == set(values), (axis, sorted({s[axis] for s in kept}), values)
    return kept


# ------------------------------------------------------------------------------------------------------------------
# normalize: k_colsum -- 16 columns per workgroup; columns below 32 * floor(N / 32) sum blocks of 16 rows, 64 blocks a round, folded
# every 16 and every 256 blocks (256 / 4096 rows); the tail columns sum four interleaved lanes (row mod 4) in blocks of 16 positions,
# 16 blocks a round, and the Nin % 4 leftover rows join lane 0 after its cascade.  k_scale_cols strides beyond 4096 x 256 elements.
NORMALIZE_SHAPES = [
    (1, 1),          # N == 1 (k_colsum_few), a single term
    (3, 5),          # Nin < 4; five columns (k_colsum_few: four on the cascade, one on row_sum)
    (3, 3),          # Nin < 4 (leftover rows only), N < 16: one partial workgroup, all tail
    (7, 33),         # Nin < 16: no complete block; Nin % 4 == 3; 32 cascade columns and ONE tail column
    (15, 16),        # Nin < 16; N == 16: exactly one workgroup, all tail; Nin % 4 == 3
    (16, 32),        # exactly one 16-row block; N % 32 == 0: no tail at all
    (17, 31),        # one block and one row; N < 32: two tail workgroups, the second partial; Nin % 4 == 1
    (18, 47),        # Nin % 4 == 2; 32 cascade columns, 15 tail columns (one partial tail workgroup)
    (19, 64),        # Nin % 4 == 3 where no column is a tail column
    (63, 1),         # N == 1: ONE column is ATen's inner reduction (k_colsum_few), 7 vectors of 8 and 7 leftover terms
    (301, 4),        # four to seven columns: the first four take the cascade, none is left for row_sum
    (4099, 7),       # ... columns 4 to 6 take row_sum; rows beyond 4096
    (1001, 8),       # and from eight columns on all are tail columns again (colsum_body)
    (255, 40),       # 15 blocks and 15 rows (below the first fold); 8 tail columns; lanes of 63 positions; Nin % 4 == 3
    (257, 65),       # 16 blocks: the first fold (a1 -> a2) and one row past it; one tail column; Nin % 4 == 1
    (1001, 37),      # 62 blocks: one round, not full; five tail columns; lanes of 250 positions (15 lane blocks); Nin % 4 == 1
    (1030, 1021),    # 64 blocks: a full round, and rows past it; 29 tail columns; Nin % 4 == 2; 1 051 630 elements: k_scale_cols' second pass
    (4097, 33),      # 256 blocks: the second fold (a2 -> a3) and one row; lanes of 1024 positions: four lane rounds, a lane fold after each
    (4099, 70),      # rows beyond 4096 with a remainder of 3 rows; six tail columns; Nin % 4 == 3
    (6403, 50),      # 400 blocks (seven rounds, the last partial) and three rows; 18 tail columns (two tail workgroups); Nin % 4 == 3
    (65539, 3),      # all tail: lanes of 16384 positions = 1024 lane blocks: the second lane fold four times; Nin % 4 == 3
    (70001, 35),     # 4375 blocks (17 second folds) and one row; three tail columns; Nin % 4 == 1
]
NORM = 78.4


def normalize_weights(Nin, N, zero_column=True):
    """Uniform [-0.2, 1.0): sums that depend on their order.  Column N // 2 is zeroed (the zero -> 1 guard)."""
    W = rng_of(11, Nin, N).uniform(-0.2, 1.0, size=(Nin, N)).astype(f32)
    if zero_column:
        W[:, N // 2] = 0.0
    return W


# ------------------------------------------------------------------------------------------------------------------
# propagation: k_prop -- 256 target columns per workgroup; sources in chunks of 1024, each of the four waves compacting its 256
# sources (four ballots of 64) into a list of at most 256 entries; entries walked four at a time; the low byte of an entry is the
# spike byte; columns from 32 * floor(N / 32) on take the row_sum order.
# one column (an inner reduction: k_prop_col1); four to seven columns (the first four on the cascade); tail only; no tail; one tail column; a
# workgroup less one, full, plus one; three workgroups
PROP_N = (1, 5, 7, 31, 32, 33, 255, 256, 257, 513)
PROP_NIN = (1, 255, 256, 257, 1023, 1024, 1025, 2049)   # one source; a wave's list less one, full, the next wave's first; a chunk less one, full, plus one; three chunks
PROP_B = (1, 3)
PROP_PATTERNS = ("p30", "ones", "last", "at1023", "bytes")


def prop_shapes():
    """(B, Nin, N): every fifth of the product, every value of every factor kept."""
    return [(B, Nin, N) for N, Nin, B in thin(itertools.product(PROP_N, PROP_NIN, PROP_B), 5, (PROP_N, PROP_NIN, PROP_B))]


def prop_inputs(B, Nin, N):
    """W, bias, the accumulate start, and the spike patterns of one shape: [(name, s u8 [B, Nin])]."""
    rng = rng_of(23, B, Nin, N)
    W = rng.uniform(-1.0, 1.0, size=(Nin, N)).astype(f32)
    bias = rng.uniform(-1.0, 1.0, size=N).astype(f32)
    prev = rng.uniform(-3.0, 3.0, size=(B, N)).astype(f32)
    dense = (rng.random((B, Nin)) < 0.3).astype(u8)
    last = np.zeros((B, Nin), u8)
    last[:, Nin - 1] = 1                                 # a single spike at i = Nin - 1
    patterns = [("p30", dense), ("ones", np.ones((B, Nin), u8)), ("last", last)]      # ones: every wave list full
    if Nin > 1023:
        at = np.zeros((B, Nin), u8)
        at[:, 1023] = 1                                  # the last slot of the first chunk (and of its fourth wave's list)
        patterns.append(("at1023", at))
    patterns.append(("bytes", dense * rng.choice(np.array([1, 2, 255], u8), size=(B, Nin))))
    return W, bias, prev, patterns


# ------------------------------------------------------------------------------------------------------------------
# narrow conv2d: k_conv2d (Cin <= 16, bank <= 64 KiB) -- dynamic LDS = the bank + up to 32 KiB of staged images of the
# 255 // (OH * OW) + 2 samples a block of 256 pixels can touch (none staged when they exceed 32 KiB: nstage == 0); 8 output channels
# per workgroup.   (B, Cin, H, W, Cout, (KH, KW), stride, pad, spike bytes)
CONV_ROWS = [
    (3, 16, 8, 8, 40, (5, 5), 1, 2, (1,)),               # bank 64 000 B + 5 images of 1024 B = 69 120 B: beyond 64 KiB of dynamic LDS
    (2, 16, 12, 12, 28, (5, 5), 1, 0, (1,)),             # 44 800 + 5 x 2304 = 56 320 B (LDS for 5 images, 2 staged): the control below 64 KiB, a bank larger than any before
    (2, 1, 130, 131, 5, (3, 3), 2, 1, (1,)),             # 2 images of 17 030 B > 32 KiB: nstage == 0, spikes from global memory
    (2, 16, 46, 47, 9, (5, 3), 1, 1, (1,)),              # 2 x 34 592 B: nstage == 0 at 16 channels, KH != KW, Cout = 8 + 1
    (300, 2, 3, 3, 3, (3, 3), 1, 0, (1,)),               # 1x1 output: a block is 256 samples, the second starts at 256 with 44 left of nstage = 257
    (3, 3, 9, 11, 7, (2, 5), 2, 1, (1,)),                # KH != KW, stride 2, Cout no multiple of 8
    (3, 4, 9, 11, 10, (3, 3), 1, 1, (1, 2, 255)),        # multi-valued spike bytes
]
CONV_DENSITIES = (0.3, 1.0)


def conv_lds_bytes(row):
    """What snn_prop_conv2d_f32 asks for: (bank bytes, nstage, total dynamic LDS)."""
    B, Cin, H, Wd, Cout, (KH, KW), stride, pad, _ = row
    OH, OW = (H + 2 * pad - KH) // stride + 1, (Wd + 2 * pad - KW) // stride + 1
    bank = 4 * Cout * Cin * KH * KW
    nstage = 255 // (OH * OW) + 2
    if nstage * Cin * H * Wd > 32 * 1024:
        nstage = 0
    return bank, nstage, bank + nstage * Cin * H * Wd


def conv_inputs(row):
    """W, bias and [(density, s)] of one row."""
    B, Cin, H, Wd, Cout, (KH, KW), stride, pad, values = row
    rng = rng_of(31, B, Cin, H, Wd, Cout, KH, KW)
    W, bias = rng.standard_normal((Cout, Cin, KH, KW)).astype(f32), rng.standard_normal(Cout).astype(f32)
    spikes = []
    for density in CONV_DENSITIES:
        s = (rng.random((B, Cin, H, Wd)) < density).astype(u8)
        spikes.append((density, s * rng.choice(np.array(values, u8), size=s.shape)))
    return W, bias, spikes


# ------------------------------------------------------------------------------------------------------------------
# Input and LIF steps: k_lif strides beyond 4096 x 256 = 1 048 576 elements, k_input beyond 2048 x 256 = 524 288.
LIF_SHAPES = [
    (1, 1),              # one thread of one workgroup
    (1, 255),            # a workgroup less one
    (3, 257),            # three workgroups and three elements; rows that are no multiple of anything
    (32, 32768),         # exactly the grid cap: 4096 workgroups, one pass
    (33, 32768),         # past it: the first 32768 elements take a second pass
    (1, 1048577),        # one element past the cap
]
INPUT_SHAPES = [
    (1, 1),
    (16, 32768),         # exactly 2048 x 256
    (1, 524289),         # one element past it
]
NODE_STEPS = 6
LIF_KW = dict(decay=float(np.exp(f32(-1.0 / 100.0))), rest=-60.0, reset=-45.0, thresh=-40.0, refrac0=2.0, lbound=-62.0)
TRACE_KINDS = [dict(trace_decay=float(np.exp(f32(-1.0 / 20.0))), trace_scale=1.0, additive=False),
               dict(trace_decay=float(np.exp(f32(-1.0 / 20.0))), trace_scale=0.5, additive=True)]


def lif_currents(B, N):
    """Uniform [-2, 6) like test_lif_and_input_vs_golden: neurons spike, sit out the refractory period and run into lbound."""
    return rng_of(41, B, N).uniform(-2.0, 6.0, size=(NODE_STEPS, B, N)).astype(f32)


def lif_thresholds(N):
    return rng_of(43, N).uniform(-48.0, -38.0, size=N).astype(f32)


def input_spikes(B, N):
    return (rng_of(47, B, N).random((NODE_STEPS, B, N)) < 0.1).astype(u8)


# ------------------------------------------------------------------------------------------------------------------
# Diehl&Cook step: k_dc_membrane -- 256 neurons per workgroup; k_dc_arbitrate -- one workgroup per sample, 256 threads striding over
# N (four waves of 64), the rows with a crossing ranked one wave per row, the last workgroup publishing the cursor.
DC_N = (1, 63, 64, 65, 255, 256, 257, 600)               # one; a wave less one, full, plus one; a stride less one, full, plus one; three strides
DC_B = (1, 5, 33)                                        # one row; rows on two ranking rounds of four waves; nine rounds
DC_STEPS = 5
DC_KW = dict(decay=float(np.exp(f32(-1.0 / 100.0))), rest=-65.0, reset=-60.0, thresh=-52.0, refrac0=1.0,
             theta_decay=float(np.exp(f32(-1.0 / 1e7))), theta_plus=0.05, trace_decay=float(np.exp(f32(-1.0 / 20.0))))


def dc_shapes():
    """(B, N): every second of the product (every value kept), and 300 rows of 257."""
    return [(B, N) for N, B in thin(itertools.product(DC_N, DC_B), 2, (DC_N, DC_B))] + [(300, 257)]


def dc_inputs(B, N):
    """Currents [5, B, N] and the noise stream.  Step 0: every row crosses; 1: none does; 2: only row 0; 3: only row B - 1; 4: every
    row again (refrac = 1: a neuron that crossed sits out one step)."""
    rng = rng_of(53, B, N)
    I = rng.uniform(-3.0, 0.0, size=(DC_STEPS, B, N)).astype(f32)
    for t, rows in ((0, range(B)), (2, [0]), (3, [B - 1]), (4, range(B))):
        for b in rows:
            I[t, b] = rng.uniform(0.0, 30.0, size=N).astype(f32)      # about half the row crosses (13 mV to go)
            I[t, b, (7 * t + b) % N] = 60.0                           # and one neuron certainly does
    Q = rng.exponential(1.0, size=(2 * B + 2) * N).astype(f32) + f32(1e-3)
    return I, Q


# ties: N = 600, B = 2.  (lower j, higher j, what the pair exercises); thread = j % 256, wave = (j % 256) // 64
DC_TIES = [
    (70, 100, "both in wave 1: the wave reduction's oj < bj"),
    (10, 74, "j and j + 64: waves 0 and 1, the cross-wave fold keeps wave 0"),
    (10, 266, "j and j + 256: one thread's two strides, strict > keeps the first"),
    (5, 200, "wave 0 and wave 3, the lower j in wave 0"),
    (200, 260, "wave 3 and wave 0 with the lower j in wave 3: the fold's red_j[w] < bj"),
]
DC_TIE_N, DC_TIE_B = 600, 2


def dc_tie_inputs(lo, hi):
    """Currents under which row 0 crosses everywhere and row 1 on every third neuron and on lo and hi; Q with its smallest value
    (0.25: 1 / q = 4 exactly) at lo and hi of both rows' draws."""
    rng = rng_of(59, lo, hi)
    I = np.zeros((DC_TIE_B, DC_TIE_N), f32)
    I[0] = 60.0
    I[1, ::3] = 60.0
    I[1, [lo, hi]] = 60.0
    Q = rng.uniform(1.0, 2.0, size=DC_TIE_B * DC_TIE_N).astype(f32)
    for b in range(DC_TIE_B):
        Q[b * DC_TIE_N + lo] = Q[b * DC_TIE_N + hi] = 0.25
    return I, Q


# ------------------------------------------------------------------------------------------------------------------
# scalar plasticity: k_plasticity<TJ>, tiles of kTI = 16 rows x TJ columns; launch_plasticity picks the widest TJ whose dynamic LDS
# (below) fits 64 KiB, 32 up to 144 KiB, and refuses beyond B = 256.
K_TI = 16


def plasticity_lds(B, TJ):
    MW = (B + 31) // 32
    return B * TJ * 4 + B * K_TI * 4 + (TJ + K_TI) * MW * 4 + B * TJ + B * K_TI


def plasticity_tile(B):
    for TJ in (256, 128, 64):
        if plasticity_lds(B, TJ) <= 64 * 1024:
            return TJ
    assert plasticity_lds(B, 32) <= 144 * 1024
    return 32


# B: either side of each tile threshold, and the largest batch        B -> TJ as launch_plasticity chooses it at this commit
PLASTICITY_B = {46: 256, 47: 128, 88: 128, 89: 64, 159: 64, 160: 32, 256: 32}
PLASTICITY_NIN = (15, 17, 33)                            # a partial tile of rows; a tile and one row; two tiles and one row
WMIN, WMAX, WDECAY = 0.1, 0.9, 0.99


def plasticity_shapes(B):
    """(B, Nin, N) with N = 2 TJ + 3 (three column tiles, the last of three columns) and N = TJ (exactly one)."""
    TJ = plasticity_tile(B)
    return [(B, Nin, N) for N in (2 * TJ + 3, TJ) for Nin in PLASTICITY_NIN]


def plasticity_inputs(B, Nin, N, inside=False, sparse=False):
    """W [0, 1) (inside: [WMIN, WMAX)), spikes (sparse: a few per step, so that whole rows, columns and tiles stay silent) and traces."""
    rng = rng_of(61, B, Nin, N, inside, sparse)
    W = (rng.uniform(WMIN, WMAX, size=(Nin, N)) if inside else rng.random((Nin, N))).astype(f32)
    ps, pt = (0.3 / B, 0.3 / B) if sparse else (0.3, 0.2)
    s_src, s_tgt = (rng.random((B, Nin)) < ps).astype(u8), (rng.random((B, N)) < pt).astype(u8)
    x_src, x_tgt = rng.random((B, Nin)).astype(f32), rng.random((B, N)).astype(f32)
    return W, s_src, x_src, s_tgt, x_tgt


MSTDP_STEPS = 3
MSTDP_KW = dict(nu0=0.02, a_plus=1.0, a_minus=-1.0, decay_plus=float(np.exp(f32(-1.0 / 20.0))), decay_minus=float(np.exp(f32(-1.0 / 20.0))))
MSTDP_CAP = (256, 2053, 16)      # B (Nin + N) = 529 664 > 2048 x 256: k_mstdp_traces' second pass
MSTDPET_CAP = (1030, 1021)       # 1 051 630 elements > 4096 x 256: k_mstdpet's second pass


def mstdp_inputs(B, Nin, N):
    """W, the spikes of MSTDP_STEPS steps and a per-sample reward vector."""
    rng = rng_of(67, B, Nin, N)
    W = rng.random((Nin, N)).astype(f32)
    s_src, s_tgt = (rng.random((MSTDP_STEPS, B, Nin)) < 0.2).astype(u8), (rng.random((MSTDP_STEPS, B, N)) < 0.2).astype(u8)
    reward_vec = rng.uniform(-1.0, 1.0, size=B).astype(f32)
    return W, s_src, s_tgt, reward_vec
