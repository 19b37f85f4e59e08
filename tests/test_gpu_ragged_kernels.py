"""The kernels of the ragged RMVPE pass at kernel level (include/rvcx_test.h): the BiGRU with a step count per sequence
(rvcx_gru_bidir_v) and the U-Net's 3x3 convs and up-convs with a height per image (rvcx_conv2d3x3_v,
rvcx_convtranspose2d_s2_v).

BiGRU: every sequence of a launch must be bit-identical to rvcx_gru_bidir on that sequence alone with T = T_b (the same
arithmetic in the same order: the per-sequence length only moves the loop bound and the reverse direction's first row).
Output rows past T_b are unspecified and not compared.

Convs: B = 3 images of heights (H_max, 1, H_max - 1) in one launch, NaN planted in every input row from an image's own
height on. A tap that read one of them would make a valid output's sum NaN, which the kernels' ReLU epilogue (v > 0 ? v
: 0) stores as 0: a grossly wrong value (measured with the bound disabled: 0.25 .. 0.88 of sum |x w| at every case),
or NaN where an epilogue lets it through. So every image's valid rows are asserted finite (image by image and mode by
mode, before anything is folded into a maximum, which would drop a NaN) and then held against float64 of that image cut to
its height, with tests/test_gpu_conv_math.py's own bar at its own shapes -- within 1e-6 of each output's sum |x w|
(+ |bias|), and the split arithmetic at most 4x the exact-f32 form's error + 1e-8. The families reached:
conv2d_small.hip's two kernels (C 16 / 32 at W = 128 and 64), conv_gemm.hip and conv_emu.hip's 2-D forms and the
windowed gather-streamed kernel (the deep shapes at W <= 32), conv_tiny.hip's two kernels (C_in = 1: the U-Net's first
conv on the mel image, whose bound is read for a wave's first output, and the launch's refusal of a shape at which a
wave would straddle two images), and the gather-streamed kernel's 2x2-phase up-conv, whose tap at h + 1 must read zero
at an image's last row.

Every case is milliseconds on the device. No test sets RVCX_GRU_SPIN_LIMIT; every test ends with a clean device status.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 256


# ----------------------------------------------------------------- BiGRU
def gru_case(T, seed):
    rng = np.random.default_rng(seed)
    gi = rng.standard_normal((len(T), max(T), 6 * H)).astype(np.float32)
    w = [rng.uniform(-1 / 16, 1 / 16, s).astype(np.float32) for s in ((3 * H, H), (3 * H,), (3 * H, H), (3 * H,))]
    return gi, w


def check_gru_rows(engine, T, seed, tag_start=0):
    gi, w = gru_case(T, seed)
    out = engine.host(engine.gru_bidir_v(gi, T, *w, tag_start=tag_start))
    engine.check_device_status()
    assert out.shape == (len(T), max(T), 2 * H)
    for b, Tb in enumerate(T):
        one = engine.host(engine.gru_bidir(gi[b:b + 1, :Tb], *w, tag_start=0))[0]
        engine.check_device_status()
        assert np.isfinite(one).all()
        assert np.array_equal(out[b, :Tb], one), f"sequence {b} (T = {Tb} of {max(T)}) differs from the run on it alone"


def test_gru_lengths_1_32_33(engine):
    check_gru_rows(engine, (1, 32, 33), seed=1)


def test_gru_17_sequences_cross_the_16_sequence_slices(engine):
    """Slice 0 (sequences 0..15) holds the shortest (1) and the longest (64) sequence; slice 1 is sequence 16 alone,
    shorter than the row stride."""
    rng = np.random.default_rng(2)
    T = [int(v) for v in rng.integers(2, 64, size=17)]
    T[3], T[11], T[16] = 1, 64, 37
    check_gru_rows(engine, T, seed=3)


@pytest.mark.parametrize("room", [2, 0])
def test_gru_tags_near_the_end_of_the_tag_space(engine, room):
    """tag_start = 2^32 - T_max - room: with room 2 the launch's last tag is 2^32 - 1 (no wrap), with room 0 the T_max
    + 1 tags would pass 2^32, so the slice is zeroed and restarts at 1."""
    T = (5, 33, 17)
    check_gru_rows(engine, T, seed=4, tag_start=2 ** 32 - max(T) - room)


# ----------------------------------------------------------------- 3x3 convs and up-convs
def planted(rng, heights, W, C):
    """x [B][H_max][W][C] with NaN in every row from an image's own height on."""
    x = rng.standard_normal((len(heights), max(heights), W, C)).astype(np.float32)
    for b, h in enumerate(heights):
        x[b, h:] = np.nan
    return x


def errs_vs_fp64(y_by_mode, heights, refs, scale=1):
    """max over images and valid rows of |y - ref| / mag, per mode. Every image's valid rows must be finite first: a
    planted row that a tap read shows as NaN there (Python's max(e, nan) would silently keep e)."""
    errs, read_past = {}, []
    for mode, y in y_by_mode.items():
        per_image = []
        for b, h in enumerate(heights):
            ref, mag = refs[b]
            got = y[b, : scale * h]
            assert got.shape == ref.shape, (mode, b, got.shape, ref.shape)
            bad = int((~np.isfinite(got)).sum())
            if bad:
                read_past.append(f"math {mode}, image {b} (height {h} of {max(heights)}): {bad} of {got.size}")
            per_image.append(float(np.max(np.abs(got - ref) / mag)))
        errs[mode] = float("nan") if np.isnan(per_image).any() else max(per_image)
    assert not read_past, ("valid outputs that are not finite (a tap read a row past the image's own height): "
                           + "; ".join(read_past))
    assert np.isfinite(list(errs.values())).all(), errs
    return errs


SMALL2D = [(64, 128, 16, 16), (48, 128, 16, 32), (40, 64, 32, 32), (40, 64, 32, 16), (33, 128, 16, 3)]
DEEP2D = [(49, 4, 512, 512), (98, 8, 256, 256), (196, 16, 128, 128), (33, 8, 256, 80), (20, 32, 128, 64)]
# C_in = 1 (conv_tiny.hip): N = 16 is the one-thread-per-row kernel (the U-Net's first conv, 1 -> 16 on the mel image),
# N = 3 the one-thread-per-output kernel; 33 rows of 128 are more than one block and no multiple of a block
TINY2D = [(33, 128, 1, 16), (33, 128, 1, 3)]


@pytest.mark.parametrize("Hm,W,C,N", SMALL2D + DEEP2D + TINY2D)
def test_conv2d3x3_per_image_heights(engine, Hm, W, C, N):
    """math "f32" and "default" at every shape (the few-channel kernels; at the deep shapes the LDS-staged fp32 and
    bf16-split 2-D forms; at C_in = 1 both codes take the same exact-fp32 one-thread kernels), and "gsw" (the windowed
    kernel) at the deep ones."""
    deep = W <= 32
    heights = (Hm, 1, Hm - 1)
    rng = np.random.Generator(np.random.PCG64(Hm * 131 + W + C + N))
    x = planted(rng, heights, W, C)
    w = (rng.standard_normal((N, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    wd, bd = torch.from_numpy(w.astype(np.float64)), torch.from_numpy(bias.astype(np.float64))
    refs = []
    for b, h in enumerate(heights):
        xd = torch.from_numpy(x[b, :h].astype(np.float64)).permute(2, 0, 1)[None]
        ref = torch.relu(torch.nn.functional.conv2d(xd, wd, bd, padding=1))[0].permute(1, 2, 0).numpy()
        mag = torch.nn.functional.conv2d(xd.abs(), wd.abs(), None, padding=1)[0].permute(1, 2, 0).numpy()
        refs.append((ref, mag + np.abs(bias)[None, None, :] + 1e-300))
    modes = ("f32", "default") + (("gsw",) if deep else ())
    ys = {m: engine.host(engine.conv2d3x3_v(x, heights, w, bias, relu=True, math=m)) for m in modes}
    engine.check_device_status()
    errs = errs_vs_fp64(ys, heights, refs)
    print(f"\n2-D ragged {Hm}x{W} {C}->{N}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["f32"] < 1e-6, errs
    for m in modes[1:]:
        assert errs[m] < 1e-6 and errs[m] <= 4.0 * errs["f32"] + 1e-8, errs


def test_tiny_conv_refuses_a_wave_that_straddles_two_images(engine):
    """conv_tiny.hip reads the height of the image a wave's first output lies in, so launch_tiny refuses per-image
    heights where an image's outputs are no multiple of 64 (here 5 x 20 rows): an error, never a wrong bound. The same
    shape without heights of its own (rvcx_conv2d3x3) runs."""
    from rvcx._lib import RvcxError

    rng = np.random.Generator(np.random.PCG64(7))
    x = rng.standard_normal((2, 5, 20, 1)).astype(np.float32)
    w = rng.standard_normal((16, 1, 3, 3)).astype(np.float32)
    with pytest.raises(RvcxError):
        engine.conv2d3x3_v(x, (5, 3), w, None, relu=True, math="f32")
    y = engine.host(engine.conv2d3x3(x[0], w, None, relu=True, math="f32"))
    assert y.shape == (5, 20, 16) and np.isfinite(y).all()
    engine.check_device_status()


UPCONV = [(49, 4, 512, 256), (98, 8, 256, 128), (196, 16, 128, 64), (392, 32, 64, 32), (33, 8, 256, 40)]


@pytest.mark.parametrize("Hm,W,C,N", UPCONV)
def test_convtranspose2d_s2_per_image_heights(engine, Hm, W, C, N):
    """The 2x2-phase up-conv: output rows 2 h + 1 of an image's last row h = H_b - 1 take the tap at h + 1, which must
    read zero (the ConvTranspose's output padding there), not the planted NaN."""
    heights = (Hm, 1, Hm - 1)
    rng = np.random.Generator(np.random.PCG64(Hm * 11 + W + C + N))
    x = planted(rng, heights, W, C)
    w = (rng.standard_normal((C, N, 3, 3)) / np.sqrt(9 * C)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    wd, bd = torch.from_numpy(w.astype(np.float64)), torch.from_numpy(bias.astype(np.float64))
    ct = torch.nn.functional.conv_transpose2d
    refs = []
    for b, h in enumerate(heights):
        xd = torch.from_numpy(x[b, :h].astype(np.float64)).permute(2, 0, 1)[None]
        ref = torch.relu(ct(xd, wd, bd, stride=2, padding=1, output_padding=1))[0].permute(1, 2, 0).numpy()
        mag = ct(xd.abs(), wd.abs(), None, stride=2, padding=1, output_padding=1)[0].permute(1, 2, 0).numpy()
        refs.append((ref, mag + np.abs(bias)[None, None, :] + 1e-300))
    ys = {m: engine.host(engine.convtranspose2d_s2_v(x, heights, w, bias, relu=True, math=m)) for m in ("f32", "default")}
    engine.check_device_status()
    errs = errs_vs_fp64(ys, heights, refs, scale=2)
    print(f"\nup-conv ragged {Hm}x{W} {C}->{N}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["f32"] < 1e-6, errs
    assert errs["default"] < 1e-6 and errs["default"] <= 4.0 * errs["f32"] + 1e-8, errs
