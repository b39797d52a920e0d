"""GPU: Phase B on the device (webp_amd/csrc/tokens.hip: wg_encode_token_stats,
wg_encode_tokens) against the serial restatement (tests/phase_b.py), and the
whole lossy encoder to a file (frames.encode_webp).

(e) Synthetic wg_mb_enc records (phase_b.synthetic_records): stats, proba_out,
    summary, hdr and the token bytes are compared for equality.  Grids: 1x1,
    3x2, 5x5, 17x4 (a row longer than a wave's worth of blocks) and 40x23
    (15 workgroups an image: the LDS histogram is flushed from several, and the
    scan's 256 lanes take four MBs each), two seeds each; a batch of three
    distinct images; a proba_in other than CoeffsProba0 with a per-image pitch.
(f) Buffer guard: a tokens_pitch a few MBs short, a canary after it.
(g) End to end: frames.encode_webp's bytes equal wg_vp8_emit of the
    restatement run on the same GPU wg_mb_enc records, and the file, parsed
    and decoded on the GPU, meets the reference's round-trip floors
    (TestLossyRoundtrip_PSNR encode_test.go:1602-1611: rich 128x64 >= 25 dB
    global and per channel, max |delta| <= 80; TestGoEncCDecLossy
    roundtrip_test.go:95-121: gradient >= 30 dB).
"""
import functools

import numpy as np
import pytest
import torch

import encode_quality as EQ
import phase_b as PB

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (3, 2), (5, 5), (17, 4), (40, 23)]
IMAGES = {"rich": EQ.rich_image, "gradient": EQ.gradient_image}
OPTS = {"zero_opts": EQ.ZERO_OPTS_Q75, "default_opts": EQ.DEFAULT_OPTS_Q75}
CASES = [("rich", 128, 64), ("gradient", 75, 70), ("gradient", 33, 65)]


@functools.lru_cache(maxsize=None)
def reference(mbw, mbh, seed, proba_seed=None):
    """(records, restatement outputs, proba_in) -- computed once, read-only."""
    enc = PB.synthetic_records(mbw, mbh, seed)
    proba_in = None
    if proba_seed is not None:
        proba_in = np.random.default_rng(proba_seed).integers(1, 256, 1056).astype(np.uint8)
        proba_in.setflags(write=False)
    pb = PB.phase_b(enc, mbw, mbh, proba_in)
    enc.setflags(write=False)
    for v in pb.values():
        v.setflags(write=False)
    return enc, pb, proba_in


def run_gpu(cuda, encs, mbw, mbh, proba=None, tokens_pitch=None):
    from webp_amd import frames
    raw = np.concatenate([np.ascontiguousarray(e).view(np.uint8).reshape(-1, 864) for e in encs])
    dev = torch.from_numpy(raw.copy()).to(cuda)
    hdr, proba_out, summ, tokens, stats = frames.encode_tokens(dev, mbw, mbh, proba=proba, tokens_pitch=tokens_pitch)
    torch.cuda.synchronize()
    return (hdr.cpu().numpy().view(PB.MB_HDR_DTYPE).reshape(len(encs), -1), proba_out.cpu().numpy(), summ,
            tokens.cpu().numpy(), stats.cpu().numpy().view(np.uint32))


def check_image(pb, hdr, proba_out, summ, tokens, stats):
    assert (stats.astype(np.int64) == pb["stats"]).all(), "stats"
    assert (proba_out == pb["proba"]).all(), "proba_out"
    assert summ.tobytes() == pb["summary"][0].tobytes(), (summ, pb["summary"])
    assert hdr.tobytes() == pb["hdr"].tobytes(), "hdr"
    n = pb["tokens"].size
    assert (tokens[:n] == pb["tokens"]).all(), "token bytes"


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("mbw,mbh", GRIDS)
def test_tokens_match_the_serial_restatement(cuda, mbw, mbh, seed):
    enc, pb, _ = reference(mbw, mbh, 100 * seed + mbw)
    hdr, proba_out, summ, tokens, stats = run_gpu(cuda, [enc], mbw, mbh)
    assert tokens.shape[1] == (pb["tokens"].size + 3) // 4 * 4  # the wrapper allocates exactly (to a dword)
    check_image(pb, hdr[0], proba_out[0], summ[0], tokens[0], stats[0])


def test_tokens_batch_of_distinct_images(cuda):
    mbw, mbh = 5, 5
    refs = [reference(mbw, mbh, s) for s in (7, 8, 9)]
    hdr, proba_out, summ, tokens, stats = run_gpu(cuda, [r[0] for r in refs], mbw, mbh)
    for k, (_, pb, _) in enumerate(refs):
        check_image(pb, hdr[k], proba_out[k], summ[k], tokens[k], stats[k])
    assert len({tokens[k].tobytes() for k in range(3)}) == 3
    assert len({int(summ[k]["total_tokens"]) for k in range(3)}) == 3


def test_tokens_with_per_image_input_probabilities(cuda):
    mbw, mbh = 5, 5
    refs = [reference(mbw, mbh, 21, proba_seed=5), reference(mbw, mbh, 22, proba_seed=6)]
    proba = np.stack([r[2] for r in refs])
    hdr, proba_out, summ, tokens, stats = run_gpu(cuda, [r[0] for r in refs], mbw, mbh, proba=proba)
    for k, (_, pb, pin) in enumerate(refs):
        check_image(pb, hdr[k], proba_out[k], summ[k], tokens[k], stats[k])
        # entries optimizeProba left alone carry proba_in, not CoeffsProba0
        assert ((proba_out[k] == pin) & (pin != PB.PROBA0)).any()


def test_tokens_short_buffer_writes_only_whole_macroblocks(cuda):
    """tokens_pitch a few MBs short: every MB whose range fits is written as
    the restatement has it, nothing else is touched (the image's tail and the
    next image's region -- here a canary image -- keep their bytes)."""
    from webp_amd import frames
    mbw, mbh = 5, 5
    enc, pb, _ = reference(mbw, mbh, 3)
    hdr_e = pb["hdr"]
    live = np.flatnonzero(hdr_e["tok_count"] > 0)
    cut = live[-3]                                 # the last three MBs with tokens do not fit
    pitch = (2 * int(hdr_e["tok_start"][cut]) + 2 * int(hdr_e["tok_count"][cut]) - 4) & ~3  # ends inside MB `cut`
    assert pitch > 2 * int(hdr_e["tok_start"][cut])
    assert 2 * (int(hdr_e["tok_start"][cut]) + int(hdr_e["tok_count"][cut])) > pitch
    raw = torch.from_numpy(np.ascontiguousarray(enc).view(np.uint8).reshape(-1, 864).copy()).to(cuda)
    n_mb = mbw * mbh
    work = torch.empty(frames.lib.wg_encode_tokens_work_bytes(mbw, mbh, 1), dtype=torch.uint8, device=cuda)
    proba_out = torch.empty(1056, dtype=torch.uint8, device=cuda)
    hdr = torch.empty((n_mb, 32), dtype=torch.uint8, device=cuda)
    summary = torch.empty(16, dtype=torch.uint8, device=cuda)
    canary = 4096
    buf = torch.full((pitch + canary,), 0xA5, dtype=torch.uint8, device=cuda)
    s = torch.cuda.current_stream().cuda_stream
    frames.call("wg_encode_token_stats", raw.data_ptr(), mbw, mbh, 1, frames.default_proba(cuda).data_ptr(), 0, None,
                proba_out.data_ptr(), hdr.data_ptr(), summary.data_ptr(), work.data_ptr(), s)
    frames.call("wg_encode_tokens", raw.data_ptr(), mbw, mbh, 1, proba_out.data_ptr(), hdr.data_ptr(), work.data_ptr(),
                buf.data_ptr(), pitch, s)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert hdr.cpu().numpy().tobytes() == hdr_e.tobytes()   # stats == NULL changes nothing else
    assert (got[pitch:] == 0xA5).all(), "canary"
    expected = np.full(pitch, 0xA5, np.uint8)
    written = 0
    for i in range(n_mb):
        a, b = 2 * int(hdr_e["tok_start"][i]), 2 * (int(hdr_e["tok_start"][i]) + int(hdr_e["tok_count"][i]))
        if b <= pitch:
            expected[a:b] = pb["tokens"][a:b]
            written += b > a
    assert written == len(live) - 3
    assert (got[:pitch] == expected).all()


def test_token_entry_points_validate_their_arguments(cuda):
    from webp_amd._lib import lib
    assert lib.wg_encode_tokens_work_bytes(800, 800, 1) == 0            # 640000 MBs x 7600 tokens > 2^32
    assert lib.wg_encode_tokens_work_bytes(565, 1000, 1) > 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=cuda)
    p = buf.data_ptr()
    assert lib.wg_encode_token_stats(p, 800, 800, 1, p, 0, None, p, p, p, p, None) == -1
    assert lib.wg_encode_token_stats(p, 1, 1, 1, None, 0, None, p, p, p, p, None) == -1
    assert lib.wg_encode_tokens(p, 1, 1, 1, p, p, p, p, 6, None) == -1     # pitch not a multiple of 4
    assert lib.wg_encode_tokens(p, 1, 1, 1, p, p, p, p + 2, 8, None) == -1  # tokens not 4-byte aligned


# --- (g) end to end -------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def encoded(name, w, h, opts, sharp):
    """frames.encode_webp's file, and wg_vp8_emit of the restatement run on the same GPU records."""
    from webp_amd import frames
    cuda = torch.device("cuda:0")
    rgba = torch.from_numpy(IMAGES[name](w, h)[None]).to(cuda)
    cfg = frames.encoder_config(**OPTS[opts])
    data = frames.encode_webp(rgba, cfg=cfg, use_sharp_yuv=sharp)[0]
    out, _, _, _, info = frames.encode_frames(rgba, cfg=cfg, use_sharp_yuv=sharp)
    enc = out.cpu().numpy().view(frames.MB_ENC_DTYPE).reshape(-1)
    mbw, mbh = frames.mb_dims(w, h)
    pb = PB.phase_b(enc, mbw, mbh)
    expect = frames.vp8_emit(w, h, cfg, info.cpu().numpy()[0], pb["hdr"], pb["proba"], pb["summary"], pb["tokens"])
    return data, expect


def decode_file(cuda, data, w, h):
    from webp_amd import frames
    dims, mb, co = frames.vp8_parse(data)
    assert (dims["width"], dims["height"]) == (w, h)
    return frames.decode_frames(frames.mb_info_tensor(mb, cuda), torch.from_numpy(co).to(cuda), dims["filter_type"],
                                dims["mbw"], dims["mbh"], 1, check=True)


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("opts", list(OPTS))
@pytest.mark.parametrize("name,w,h", CASES)
def test_encode_webp_end_to_end(cuda, name, w, h, opts, sharp):
    from webp_amd import frames
    data, expect = encoded(name, w, h, opts, sharp)
    assert data == expect, "encode_webp's bytes differ from the emitter over the restatement's tokens"
    Y, U, V = decode_file(cuda, data, w, h)
    src = IMAGES[name](w, h)
    if name == "rich":   # TestLossyRoundtrip_PSNR
        y, u, v = (p[0].cpu().numpy() for p in (Y, U, V))
        per, glob, maxd = EQ.rgb_channel_stats(src[..., :3], EQ.go_ycbcr_rgb(y, u, v, w, h))
        print(f"rich {w}x{h} {opts} sharp={sharp}: global {glob:.2f} dB, per channel {per}, max delta {maxd}")
        assert glob >= 25.0 and min(per) >= 25.0 and max(maxd) <= 80
    else:                # TestGoEncCDecLossy
        dec = frames.build_nrgba(Y, U, V, w, h)[0].cpu().numpy()
        p = EQ.rgba_psnr(src, dec)
        print(f"gradient {w}x{h} {opts} sharp={sharp}: {p:.2f} dB")
        assert p >= 30.0
