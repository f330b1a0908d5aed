"""Shared by tests/test_gpu_conv_mfma.py and tests/test_conv_mfma_hostcheck.py: the shapes and the numpy restatement of the stated order."""
import numpy as np

# (Cin, Cout, K or (KH, KW), stride, pad, H, W, B): per-tap channel padding with partial tiles; several channel groups, stride, a block spanning
# samples; OH*OW = 16; windows mostly outside the image; padded K of 576 (several slabs); a bank beyond 64 KiB with few channels;
# 1024 workgroups of two channel tiles per wave (the other instance); 96 KiB of bands (a launch beyond the default 64 KiB of LDS);
# the tap walk it shares with snn_run_conv2d_sif_f32 where KH != KW (taller, wider and a single row, with a stride) and where the
# padding is beyond half the kernel (OH > H, most of a border window outside)
SHAPES = [(17, 5, 3, 1, 1, 5, 5, 1), (32, 80, 3, 2, 1, 9, 7, 3), (48, 16, 1, 1, 0, 4, 4, 5), (20, 17, 5, 1, 2, 6, 6, 2),
          (64, 32, 3, 1, 1, 8, 8, 1), (4, 300, 7, 1, 0, 9, 9, 2), (20, 40, 1, 1, 0, 128, 128, 2), (17, 5, 3, 1, 1, 4, 512, 1),
          (17, 5, (5, 3), 1, 1, 9, 7, 2), (17, 20, (1, 3), 2, 1, 9, 7, 3), (20, 5, (3, 5), 2, 2, 9, 7, 2), (17, 5, 3, 1, 2, 5, 5, 2)]


def khw(K):
    return (K, K) if isinstance(K, int) else tuple(K)


def case(shape, seed=0, levels=2, density=0.3):      # randn weights and bias, Bernoulli spikes with bytes 1 .. levels - 1, the output shape
    Cin, Cout, K, stride, pad, H, Wd, B = shape
    rs = np.random.RandomState(seed + Cin * 1000 + Cout)
    (KH, KW) = khw(K)
    W, bias = rs.randn(Cout, Cin, KH, KW).astype(np.float32), rs.randn(Cout).astype(np.float32)
    s = ((rs.uniform(size=(B, Cin, H, Wd)) < density) * rs.randint(1, levels, size=(B, Cin, H, Wd))).astype(np.uint8)
    return W, bias, s, (B, Cout, (H + 2 * pad - KH) // stride + 1, (Wd + 2 * pad - KW) // stride + 1)


def stated_order(W, s, bias, stride, pad, prev=None):
    """Every output's sequential float32 sum over (ky, kx, ci), a rounded multiply and a rounded add per non-zero byte, bias last (a
    zero byte adds nothing: padding with zeros is skipping the out-of-image taps)."""
    (B, Cin, H, Wd), (Cout, _, KH, KW) = s.shape, W.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (Wd + 2 * pad - KW) // stride + 1
    sp = np.zeros((B, Cin, H + 2 * pad, Wd + 2 * pad), np.uint8)
    sp[:, :, pad:pad + H, pad:pad + Wd] = s
    acc = np.zeros((B, Cout, OH, OW), np.float32)
    for ky, kx, ci in np.ndindex(KH, KW, Cin):
        byte = sp[:, ci, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride][:, None]
        acc = np.where(byte != 0, acc + byte.astype(np.float32) * W[None, :, ci, ky, kx, None, None], acc).astype(np.float32)
    acc = acc if bias is None else acc + bias[None, :, None, None]
    return acc if prev is None else (prev + acc).astype(np.float32)
