"""GPU: wg_import_ycbcr (k_import_ycbcr) against VP8Encoder.importYCbCr
(internal/lossy/encode.go:544-585).  The reference clamps the source index
per plane (srcX = min(x, w - 1), srcY = min(y, h - 1)), which is numpy's edge
padding, so the expected planes are np.pad(plane, ..., mode="edge").

Copy mode: unaligned source (base off by one byte, row stride w + 5), three
distinct images, destination pitches 64 bytes past the planes with the gaps
checked untouched.  Sizes: 1x1 (all margin), 16x16 (no margin), odd sizes with
up to 15 margin columns / rows and odd chroma, odd mbw (8-byte last chroma
span), and a padded width past one block's 4096 columns.

In place: the interior of the padded planes is the source; the margin must
come from the interior's last column / row whatever the margin held before."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FILL = 0xA5
GAP = 64
COPY_SIZES = [(1, 1), (16, 16), (17, 33), (33, 65), (75, 70), (255, 49), (4099, 17)]
INPLACE_SIZES = [(33, 65), (75, 70), (64, 64)]


def dims(w, h):
    mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
    return mbw, mbh, (w + 1) // 2, (h + 1) // 2


def edge_pad(p, rows, cols):
    return np.pad(p, ((0, 0), (0, rows - p.shape[1]), (0, cols - p.shape[2])), mode="edge")


def random_planes(n, w, h, seed):
    _, _, cw, ch = dims(w, h)
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, h, w), dtype=np.uint8), rng.integers(0, 256, (n, ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (n, ch, cw), dtype=np.uint8))


def strided_source(plane, dev):
    """The plane in a buffer whose base is off by one byte and whose rows are w + 5 apart."""
    n, h, w = plane.shape
    stride = w + 5
    buf = torch.full((1 + n * h * stride,), 0x3C, dtype=torch.uint8, device=dev)
    view = buf[1:].view(n, h, stride)[:, :, :w]
    view.copy_(torch.from_numpy(plane).to(dev))
    assert view.data_ptr() % 2 == 1
    return buf, view


def check_copy(cuda, w, h, gap_y, gap_uv):
    from webp_amd import frames
    from webp_amd._lib import call
    n = 3
    mbw, mbh, cw, ch = dims(w, h)
    Y, U, V = random_planes(n, w, h, seed=w * 131 + h)
    keep = [strided_source(p, cuda) for p in (Y, U, V)]
    ybytes, cbytes = 256 * mbw * mbh, 64 * mbw * mbh
    bufs = [torch.full((n, nb + g), FILL, dtype=torch.uint8, device=cuda)
            for nb, g in ((ybytes, gap_y), (cbytes, gap_uv), (cbytes, gap_uv))]
    sy, su, sv = (k[1] for k in keep)
    assert su.stride() == sv.stride()
    call("wg_import_ycbcr", sy.data_ptr(), sy.stride(1), sy.stride(0), su.data_ptr(), sv.data_ptr(), su.stride(1),
         su.stride(0), w, h, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), ybytes + gap_y, cbytes + gap_uv, n,
         frames._stream())
    torch.cuda.synchronize()
    exp = (edge_pad(Y, 16 * mbh, 16 * mbw), edge_pad(U, 8 * mbh, 8 * mbw), edge_pad(V, 8 * mbh, 8 * mbw))
    for name, buf, e, nb in zip("YUV", bufs, exp, (ybytes, cbytes, cbytes)):
        got = buf.cpu().numpy()
        assert (got[:, nb:] == FILL).all(), f"{name}: bytes past the plane were written"
        assert (got[:, :nb].reshape(e.shape) == e).all(), f"{name} plane differs from the edge-padded source"
    for (buf, view), p in zip(keep, (Y, U, V)):  # the source is read only
        assert (view.cpu().numpy() == p).all() and int(buf[0]) == 0x3C


@pytest.mark.parametrize("w,h", COPY_SIZES)
def test_copy_mode_matches_edge_padding(cuda, w, h):
    check_copy(cuda, w, h, GAP, GAP)


def test_copy_mode_least_aligned_destination(cuda):
    """Pitches at the destination rules' minimum alignment (Y 8, U / V 4 bytes):
    the second and third images' rows take the 8- and 4-byte store paths."""
    check_copy(cuda, 33, 65, 8, 4)


def test_copy_mode_through_frames_import_ycbcr(cuda):
    """frames.import_ycbcr on contiguous (aligned) planes, allocating its output."""
    from webp_amd import frames
    w, h, n = 75, 70, 2
    mbw, mbh, _, _ = dims(w, h)
    Y, U, V = random_planes(n, w, h, seed=5)
    got = frames.import_ycbcr(*(torch.from_numpy(p).to(cuda) for p in (Y, U, V)))
    torch.cuda.synchronize()
    exp = (edge_pad(Y, 16 * mbh, 16 * mbw), edge_pad(U, 8 * mbh, 8 * mbw), edge_pad(V, 8 * mbh, 8 * mbw))
    for g, e in zip(got, exp):
        assert g.shape == e.shape and (g.cpu().numpy() == e).all()


# (interior, stale margin byte): a random interior under a 0xA5 prefill; the
# interior 0xA5 as well; and the interior 0xA5 under the complement, so that a
# margin byte left as it was, or taken from another stale byte, shows
INPLACE_CASES = [("random", FILL), ("fill", FILL), ("fill", FILL ^ 0xFF)]


@pytest.mark.parametrize("interior,stale", INPLACE_CASES)
@pytest.mark.parametrize("w,h", INPLACE_SIZES)
def test_in_place_fills_only_the_margin_from_the_interior(cuda, w, h, interior, stale):
    from webp_amd import frames
    n = 2
    mbw, mbh, cw, ch = dims(w, h)
    if interior == "fill":
        src = tuple(np.full(s, FILL, np.uint8) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))
    else:
        src = random_planes(n, w, h, seed=w + 7 * h)
    shapes = ((n, 16 * mbh, 16 * mbw), (n, 8 * mbh, 8 * mbw), (n, 8 * mbh, 8 * mbw))
    planes = [torch.full(s, stale, dtype=torch.uint8, device=cuda) for s in shapes]
    views = []
    for p, s in zip(planes, src):
        v = p[:, :s.shape[1], :s.shape[2]]
        v.copy_(torch.from_numpy(s).to(cuda))
        views.append(v)
    out = frames.import_ycbcr(*views, out=tuple(planes))
    torch.cuda.synchronize()
    assert all(o.data_ptr() == p.data_ptr() for o, p in zip(out, planes))
    for name, p, s, shp in zip("YUV", planes, src, shapes):
        assert (p.cpu().numpy() == edge_pad(s, shp[1], shp[2])).all(), f"{name} plane differs from the edge-padded interior"
