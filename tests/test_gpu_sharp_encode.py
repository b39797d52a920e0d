"""GPU: the UseSharpYUV encode path end to end -- webp.Encode with
EncoderOptions.UseSharpYUV (encode.go:1174-1234 sharpYUVConvert ->
lossy.NewEncoderFromYUV, internal/lossy/encode.go:500-539 -> importYCbCr
:544-585 -> analysis, segments, Phase A), on the device through
frames.sharpyuv_import_rgba and frames.encode_frames(use_sharp_yuv=True).

The expected values are the restatement's chain, built here from what the
oracle exposes: O.sharpyuv_convert of the RGB bytes, numpy edge padding to
macroblock size (importYCbCr's index clamp), O.encode_frame, the MBData the
bitstream would carry (encode_quality.mbdata_from_encoder) and
O.decode_frame.  Everything is compared bit for bit; the decoded result is
then held to the reference's own round-trip floors:

- TestLossyRoundtrip_PSNR (encode_test.go:1602-1611), richTestImage 128x64:
  global and per-channel RGB PSNR >= 25 dB and max |delta| <= 80 through Go's
  YCbCr -> RGB.  The restatement alone: 28.19 dB (zero options) and 28.26 dB
  (default options) global, max delta 28.
- TestGoEncCDecLossy (testc/roundtrip/roundtrip_test.go:95-121),
  generateGradient: RGBA PSNR >= 30 dB through the fancy upsampler.  The
  restatement alone: 128x128 39.4 / 39.9 dB, 75x70 38.5 / 37.7 dB.
"""
import functools

import numpy as np
import pytest
import torch

import encode_quality as EQ
import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("coeffs", "modes", "nz_y", "nz_uv", "non_zero_y", "non_zero_uv", "mb_type", "i16_mode", "uv_mode", "nz_dc",
          "skip", "segment", "score")  # MBEncInfo, as tests/test_gpu_bench_config.py
IMAGES = {"rich": EQ.rich_image, "gradient": EQ.gradient_image, "pattern": EQ.color_pattern}
OPTS = {"zero_opts": EQ.ZERO_OPTS_Q75, "default_opts": EQ.DEFAULT_OPTS_Q75}
PLANE_CASES = [("rich", 128, 64), ("gradient", 75, 70), ("gradient", 33, 65), ("gradient", 64, 64)]
ENCODE_CASES = [("rich", 128, 64), ("gradient", 75, 70), ("gradient", 33, 65)]
BATCH = [("gradient", 75, 70), ("rich", 75, 70), ("pattern", 75, 70)]


def with_random_alpha(rgba, seed):
    """The same pixels with the alpha bytes random: sharpYUVConvert drops alpha."""
    out = rgba.copy()
    out[..., 3] = np.random.default_rng(seed).integers(0, 256, rgba.shape[:2], dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def chain_planes(name, w, h):
    """sharpyuv.Convert + importYCbCr on the restatement: padded (Y, U, V), iterations."""
    rgba = IMAGES[name](w, h)
    Y, U, V, its = O.sharpyuv_convert(rgba[..., :3])
    mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
    pad = lambda p, rows, cols: np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")
    planes = (pad(Y, 16 * mbh, 16 * mbw), pad(U, 8 * mbh, 8 * mbw), pad(V, 8 * mbh, 8 * mbw))
    for p in planes:
        p.setflags(write=False)
    return planes, int(its)


@functools.lru_cache(maxsize=None)
def chain_encode(name, w, h, opts):
    """The rest of the chain: (mb_enc, recon planes, seg_ids, info, decoded planes)."""
    o = OPTS[opts]
    (Y, U, V), _ = chain_planes(name, w, h)
    enc, recon, ids, info = O.encode_frame(Y, U, V, w, h, O.encoder_config(**o))
    mb, co, ftype = EQ.mbdata_from_encoder(enc, info, simple=o["filter_type"] == 0,
                                           cfg_filter_strength=o["filter_strength"])
    dec = O.decode_frame(mb, co, ftype, Y.shape[1] // 16, Y.shape[0] // 16)
    return enc, recon, ids, info, dec


def to_np(planes, i=0):
    return tuple(p[i].cpu().numpy() for p in planes)


@pytest.mark.parametrize("name,w,h", PLANE_CASES)
def test_sharpyuv_import_planes_match_the_chain(cuda, name, w, h):
    from webp_amd import frames
    rgba = with_random_alpha(IMAGES[name](w, h), seed=w + h)
    dev = torch.from_numpy(rgba[None]).to(cuda)
    Y, U, V, its = frames.sharpyuv_import_rgba(dev, iterations=True)
    (ey, eu, ev), e_its = chain_planes(name, w, h)
    gy, gu, gv = to_np((Y, U, V))
    assert gy.shape == ey.shape and gu.shape == eu.shape and gv.shape == ev.shape
    assert (gy == ey).all() and (gu == eu).all() and (gv == ev).all()
    assert int(its[0]) == e_its
    # UseSharpYUV is honoured: importImage's planes of the same frame differ
    iy = frames.import_rgba(dev, has_alpha=False)[0][0].cpu().numpy()
    differ = float((iy != gy).mean())
    print(f"{name} {w}x{h}: {100 * differ:.1f} % of Y bytes differ from importImage, {e_its} iterations")
    assert differ > 0


def test_sharpyuv_import_batch_of_distinct_images(cuda):
    from webp_amd import frames
    rgba = np.stack([with_random_alpha(IMAGES[n](w, h), seed=k) for k, (n, w, h) in enumerate(BATCH)])
    Y, U, V, its = frames.sharpyuv_import_rgba(torch.from_numpy(rgba).to(cuda), iterations=True)
    for k, (n, w, h) in enumerate(BATCH):
        (ey, eu, ev), e_its = chain_planes(n, w, h)
        gy, gu, gv = to_np((Y, U, V), k)
        assert (gy == ey).all() and (gu == eu).all() and (gv == ev).all(), k
        assert int(its[k]) == e_its, k
    assert len({Y[k].cpu().numpy().tobytes() for k in range(len(BATCH))}) == len(BATCH)


def gpu_encode(cuda, name, w, h, opts):
    from webp_amd import frames
    rgba = with_random_alpha(IMAGES[name](w, h), seed=3 * w + h)
    cfg = frames.encoder_config(**OPTS[opts])
    out, recon, seg_ids, _, info = frames.encode_frames(torch.from_numpy(rgba[None]).to(cuda), cfg, check=True,
                                                        use_sharp_yuv=True)
    enc = out.cpu().numpy().view(frames.MB_ENC_DTYPE).reshape(-1)
    info = info.cpu().numpy().view(frames.FRAME_SEGS_DTYPE).reshape(-1)[0]
    return enc, to_np(recon), seg_ids[0].cpu().numpy(), info


@pytest.mark.parametrize("opts", list(OPTS))
@pytest.mark.parametrize("name,w,h", ENCODE_CASES)
def test_sharp_encode_matches_the_chain(cuda, name, w, h, opts):
    enc, recon, seg_ids, info = gpu_encode(cuda, name, w, h, opts)
    e_enc, e_recon, e_ids, e_info, _ = chain_encode(name, w, h, opts)
    assert (seg_ids == e_ids).all()
    assert info.tobytes() == e_info.tobytes()
    for f in FIELDS:
        assert (enc[f] == e_enc[f]).all(), f"field {f}"
    # exportParallel (encode_parallel.go:1412-1495) writes luma over the w x h
    # image only and chroma over whole macroblocks: that is the reconstruction
    # (as tests/test_gpu_encode.py compares it)
    assert (recon[0][:h, :w] == e_recon[0][:h, :w]).all(), "reconstructed Y"
    assert (recon[1] == e_recon[1]).all() and (recon[2] == e_recon[2]).all(), "reconstructed U / V"


def gpu_round_trip(cuda, name, w, h, opts):
    """Encode with UseSharpYUV, then decode what the bitstream carries on the
    GPU; the decoded device planes, checked bit-exact against the chain."""
    from webp_amd import frames
    o = OPTS[opts]
    enc, _, _, info = gpu_encode(cuda, name, w, h, opts)
    mb, co, ftype = EQ.mbdata_from_encoder(enc, info, simple=o["filter_type"] == 0,
                                           cfg_filter_strength=o["filter_strength"])
    mbw, mbh = frames.mb_dims(w, h)
    planes = frames.decode_frames(frames.mb_info_tensor(mb), torch.from_numpy(co).to(cuda), ftype, mbw, mbh, 1,
                                  check=True)
    e_dec = chain_encode(name, w, h, opts)[4]
    for p, (g, e) in zip("YUV", zip(to_np(planes), e_dec)):
        assert (g == e).all(), f"decoded {p}"
    return planes


@pytest.mark.parametrize("opts", list(OPTS))
def test_sharp_round_trip_lossy_psnr(cuda, opts):
    """TestLossyRoundtrip_PSNR's assertions (encode_test.go:1602-1611)."""
    src = EQ.rich_image(128, 64)
    Y, U, V = to_np(gpu_round_trip(cuda, "rich", 128, 64, opts))
    per, glob, maxd = EQ.rgb_channel_stats(src[..., :3], EQ.go_ycbcr_rgb(Y, U, V, 128, 64))
    print(f"rich 128x64 {opts}: global {glob:.2f} dB, per channel {per}, max delta {maxd}")
    assert glob >= 25.0, f"global PSNR {glob:.2f} dB < 25"
    assert max(maxd) <= 80, f"max delta {maxd} > 80"
    assert min(per) >= 25.0, f"per-channel PSNR {per} < 25"


@pytest.mark.parametrize("opts", list(OPTS))
@pytest.mark.parametrize("w,h", [(128, 128), (75, 70)])
def test_sharp_round_trip_go_enc_c_dec(cuda, w, h, opts):
    """TestGoEncCDecLossy's floor (roundtrip_test.go:95-121) through the fancy upsampler."""
    from webp_amd import frames
    src = EQ.gradient_image(w, h)
    Y, U, V = gpu_round_trip(cuda, "gradient", w, h, opts)
    dec = frames.build_nrgba(Y, U, V, w, h)[0].cpu().numpy()
    p = EQ.rgba_psnr(src, dec)
    print(f"gradient {w}x{h} {opts}: {p:.2f} dB")
    assert p >= 30.0
