"""GPU parity of the exact configuration bench.py times: 64 x 1920x1080 frames
per batch, three batches in flight on three HIP streams (4,352 encoder rows
on 2,048 resident wave slots, persistent kernels overlapping), the
reference's q75 defaults with the device segment analysis, and the libwebp q75
bitstreams on the decode side.

After four steps (slot 0 reused) every slot's in-kernel wait flags are
checked, and five frames of the batch -- the first of each content (G, N, P)
and two later ones with other seeds -- are compared bit-for-bit with the
oracle (every MBEncInfo field, the reconstruction, the segment map and
records, the decoded planes and the NRGBA).  Every frame's encode input is
distinct (bench.frame_rgba: content g % 3, seed g); the decode side replays
the three contents' streams, so every other frame's decoded planes must equal
those of the first frame of its content byte for byte."""
import os

import numpy as np
import pytest
import torch

import bench
import oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ("coeffs", "modes", "nz_y", "nz_uv", "non_zero_y", "non_zero_uv", "mb_type", "i16_mode", "uv_mode", "nz_dc",
          "skip", "segment", "score")


@pytest.fixture(scope="module")
def ran(cuda):
    rgba, mb, co, parsed = bench.make_inputs(64, 0, cuda)
    pipe = bench.Pipeline(rgba, mb, co, 64, cuda, slots=3)
    for _ in range(4):
        pipe.step()
    torch.cuda.synchronize()
    pipe.check_status()
    return rgba, parsed, pipe


def expected(content, rgba_np, parsed):
    W, H = bench.W, bench.H
    y, u, v = O.import_rgba(rgba_np, has_alpha=False)
    enc, recon, ids, info = O.encode_frame(y, u, v, W, H, O.encoder_config(**bench.ENC_CFG))
    mb, co = parsed[content]
    dy, du, dv = O.decode_frame(mb, co, 2, bench.MBW, bench.MBH)
    nrgba = O.build_nrgba(dy, du, dv, W, H)
    return enc, recon, ids, info, (dy, du, dv), nrgba


CHECKED = (0, 1, 2, 34, 63)


def test_bench_batch_matches_oracle(ran):
    from webp_amd import frames
    rgba, parsed, pipe = ran
    per = bench.MBW * bench.MBH
    exp = {}
    for i in CHECKED:
        src = rgba[i].cpu().numpy()
        assert (src == bench.frame_rgba(i)).all()
        exp[i] = expected(bench.CONTENTS[i % 3], src, parsed)
    for s, sl in enumerate(pipe.slots):
        got = sl.enc_out.cpu().numpy().view(frames.MB_ENC_DTYPE).reshape(64, per)
        info = sl.seg_info.cpu().numpy().view(frames.FRAME_SEGS_DTYPE).reshape(64)
        seg_ids = sl.seg_ids.cpu().numpy()
        planes = [t.cpu().numpy() for t in (sl.rY, sl.rU, sl.rV, sl.dY, sl.dU, sl.dV, sl.out)]
        for i in CHECKED:
            enc, (ry, ru, rv), ids, inf, (dy, du, dv), nrgba = exp[i]
            assert (seg_ids[i] == ids).all() and info[i].tobytes() == inf.tobytes(), (s, i)
            for f in FIELDS:
                assert (got[i][f] == enc[f]).all(), f"slot {s} frame {i}: field {f}"
            assert (planes[0][i][:bench.H] == ry[:bench.H]).all() and (planes[1][i] == ru).all() and \
                (planes[2][i] == rv).all(), (s, i)
            assert (planes[3][i] == dy).all() and (planes[4][i] == du).all() and (planes[5][i] == dv).all(), (s, i)
            assert (planes[6][i] == nrgba).all(), (s, i)
        # the rest of the batch: the decode side replays the three contents'
        # streams (identical inputs, identical outputs); the encode side's
        # frames all differ
        for i in range(3, 64):
            r = i % 3
            for p in planes[3:]:
                assert (p[i] == p[r]).all(), (s, i)
        raw = sl.enc_out.cpu().numpy().reshape(64, -1)
        assert len({raw[i].tobytes() for i in range(64)}) == 64, s


def test_dump_outputs_sample_the_last_step(ran, tmp_path):
    """bench.py --dump-outputs: float32 / float64 .npy files of at most 64 MB in
    all, identical from one dump to the next, holding the last step's slot:
    whole arrays where they are small, the values at bench.dump_positions
    where they are sampled."""
    from webp_amd import frames
    _, _, pipe = ran
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(pipe, a)
    bench.dump_outputs(pipe, b)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64 * 1000 * 1000
    got = {n[:-4]: np.load(os.path.join(a, n)) for n in names}
    for n in names:
        assert n.endswith(".npy") and got[n[:-4]].dtype in (np.float32, np.float64), n
        assert np.array_equal(got[n[:-4]], np.load(os.path.join(b, n))), n
    sl = pipe.slots[(pipe.k - 1) % len(pipe.slots)]
    W, H = bench.W, bench.H
    cw, ch = (W + 1) // 2, (H + 1) // 2
    planes = {"recon_y": sl.rY[:, :H, :W], "recon_u": sl.rU[:, :ch, :cw], "recon_v": sl.rV[:, :ch, :cw],
              "dec_y": sl.dY[:, :H, :W], "dec_u": sl.dU[:, :ch, :cw], "dec_v": sl.dV[:, :ch, :cw], "nrgba": sl.out,
              "segment_ids": sl.seg_ids}
    for name, t in planes.items():
        flat = t.cpu().numpy().reshape(-1)
        if flat.size > bench.DUMP_ELEMENTS:
            flat = flat[bench.dump_positions(name, flat.size, bench.DUMP_ELEMENTS)]
        assert got[name].dtype == np.float32 and np.array_equal(got[name], flat), name
    recs = sl.enc_out.cpu().numpy().view(frames.MB_ENC_DTYPE).reshape(-1)
    recs = recs[bench.dump_positions("enc", recs.size, bench.DUMP_RECORDS)]
    for f in FIELDS:
        assert np.array_equal(got["enc_" + f], recs[f]), f
    assert got["enc_score"].dtype == np.float64 and got["enc_coeffs"].shape == (bench.DUMP_RECORDS, 400)
    info = sl.seg_info.cpu().numpy().view(frames.FRAME_SEGS_DTYPE).reshape(-1)
    for f in frames.FRAME_SEGS_DTYPE.names:
        if not f.startswith("pad"):
            assert np.array_equal(got["frame_segs_" + f], info[f]), f
    assert len(got) == len(planes) + len(FIELDS) + len(frames.FRAME_SEGS_DTYPE.names) - 2
