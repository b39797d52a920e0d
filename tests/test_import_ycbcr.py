"""CPU: the UseSharpYUV import seam of the C ABI -- wg_import_ycbcr
(VP8Encoder.importYCbCr, internal/lossy/encode.go:544-585) and
wg_sharpyuv_import_rgba (sharpYUVConvert, encode.go:1174-1234, into
NewEncoderFromYUV's import) are declared, exported and bound, and reject bad
arguments on the host, before any device work (no GPU needed)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "webpgpu.h")
NEW = ("wg_import_ycbcr", "wg_sharpyuv_import_rgba")
EINVAL = -1

P = 1 << 20  # fake, well aligned device addresses, far apart: validation fails before any is dereferenced
SY, SU, SV, DY, DU, DV, WORK, RGBA = (P * k for k in range(1, 9))


def test_header_library_and_binding_have_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    from webp_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["wg_import_ycbcr"]) == 16 and len(_lib.SIGNATURES["wg_sharpyuv_import_rgba"]) == 13
    assert _lib.lib.wg_version() == 2  # symbols were only added
    from webp_amd import frames
    assert callable(frames.import_ycbcr) and callable(frames.sharpyuv_import_rgba)


def ycbcr_args(w=33, h=65, sy=SY, su=SU, sv=SV, sy_stride=None, sy_pitch=None, suv_stride=None, suv_pitch=None,
               y=DY, u=DU, v=DV, y_pitch=None, uv_pitch=None, n=1):
    mbw, mbh = (w + 15) >> 4, (h + 15) >> 4
    cw, ch = (w + 1) // 2, (h + 1) // 2
    sy_stride = max(w, 1) if sy_stride is None else sy_stride
    suv_stride = max(cw, 1) if suv_stride is None else suv_stride
    return (sy, sy_stride, sy_stride * max(h, 1) if sy_pitch is None else sy_pitch, su, sv, suv_stride,
            suv_stride * max(ch, 1) if suv_pitch is None else suv_pitch, w, h, y, u, v,
            256 * mbw * mbh if y_pitch is None else y_pitch, 64 * mbw * mbh if uv_pitch is None else uv_pitch, n, None)


def test_import_ycbcr_rejects_bad_arguments_without_a_device():
    from webp_amd import _lib
    f = _lib.lib.wg_import_ycbcr
    bad = {
        "NULL sy": ycbcr_args(sy=None), "NULL su": ycbcr_args(su=None), "NULL sv": ycbcr_args(sv=None),
        "NULL y": ycbcr_args(y=None), "NULL u": ycbcr_args(u=None), "NULL v": ycbcr_args(v=None),
        "w = 0": ycbcr_args(w=0), "w < 0": ycbcr_args(w=-3), "h = 0": ycbcr_args(h=0), "n = 0": ycbcr_args(n=0),
        "sy_stride < w": ycbcr_args(sy_stride=32), "suv_stride < cw": ycbcr_args(suv_stride=16),
        "sy_pitch < plane": ycbcr_args(sy_pitch=33 * 64), "suv_pitch < plane": ycbcr_args(suv_pitch=17 * 32),
        "y_pitch < 256*mbw*mbh": ycbcr_args(y_pitch=256 * 3 * 5 - 8), "uv_pitch < 64*mbw*mbh": ycbcr_args(uv_pitch=64 * 3 * 5 - 4),
        "y misaligned": ycbcr_args(y=DY + 2), "y_pitch % 8": ycbcr_args(y_pitch=256 * 3 * 5 + 4),
        # overlaps that are not the exact in-place form
        "same pointers, sy_stride = w": ycbcr_args(sy=DY, su=DU, sv=DV),
        "same pointers, packed pitches": ycbcr_args(sy=DY, su=DU, sv=DV, sy_stride=48, suv_stride=24, sy_pitch=48 * 65,
                                                    suv_pitch=24 * 33),
        "in-place Y, separate chroma": ycbcr_args(sy=DY, sy_stride=48, sy_pitch=256 * 3 * 5),
        "source Y inside destination Y": ycbcr_args(sy=DY + 100),
        "source U over destination V": ycbcr_args(su=DV + 8),
        "second image's source over the destination": ycbcr_args(sy=DY - 40 * 65 - 10, sy_stride=40, n=2, y_pitch=256 * 15),
    }
    for what, args in bad.items():
        assert f(*args) == EINVAL, what
        assert b"invalid argument" in _lib.lib.wg_last_error() or b"overlap" in _lib.lib.wg_last_error(), what


def test_sharpyuv_import_rgba_rejects_bad_arguments_without_a_device():
    from webp_amd import _lib
    f = _lib.lib.wg_sharpyuv_import_rgba

    def args(rgba=RGBA, w=33, h=65, stride=None, pitch=None, y=DY, u=DU, v=DV, y_pitch=256 * 15, uv_pitch=64 * 15, n=1,
             work=WORK):
        stride = 4 * max(w, 1) if stride is None else stride
        return (rgba, w, h, stride, stride * max(h, 1) if pitch is None else pitch, y, u, v, y_pitch, uv_pitch, n, work,
                None)

    bad = {
        "NULL rgba": args(rgba=None), "NULL y": args(y=None), "NULL u": args(u=None), "NULL v": args(v=None),
        "NULL work": args(work=None), "w = 0": args(w=0), "h < 0": args(h=-1), "n = 0": args(n=0),
        "stride < 4w": args(stride=4 * 33 - 1), "y_pitch < 256*mbw*mbh": args(y_pitch=256 * 15 - 8),
        "uv_pitch < 64*mbw*mbh": args(uv_pitch=64 * 15 - 4), "u misaligned": args(u=DU + 1),
        "work misaligned": args(work=WORK + 8),
    }
    for what, a in bad.items():
        assert f(*a) == EINVAL, what
