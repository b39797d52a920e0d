"""The UseSharpYUV import seam on one GPU: N x WxH RGBA frames (default
64 x 1920x1080, the flagship batch), median device time with HIP events on the
current stream after a warm-up, for

  sharpyuv_import_rgba   wg_sharpyuv_import_rgba: SharpYUV into the padded planes + the margin fill
  margin_in_place        wg_import_ycbcr in place on those planes: the margin alone
  import_ycbcr_copy      wg_import_ycbcr copy mode from unpadded planes
  import_rgba            wg_import_rgba (importImage), for scale

and the bytes each moves, computed from the shapes (read once + written once;
a replicated margin byte's source is counted once per span that reads it).
No threshold: prints one JSON line.  Environment: N, W, H, REPS."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import synth  # noqa: E402
from webp_amd import frames  # noqa: E402

N = int(os.environ.get("N", "64"))
W = int(os.environ.get("W", "1920"))
H = int(os.environ.get("H", "1080"))
REPS = int(os.environ.get("REPS", "20"))


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def moved_bytes(w, h, n):
    """Algorithmic bytes of the two import modes and of importImage."""
    mbw, mbh = frames.mb_dims(w, h)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    padded = 256 * mbw * mbh + 2 * 64 * mbw * mbh
    interior = w * h + 2 * cw * ch
    # copy: every source byte read, every padded byte written
    copy = n * (interior + padded)
    # in place: the margin written; read: the last interior row once per margin row, the last interior
    # column's byte once per row with a column margin
    mrows_y, mrows_c = 16 * mbh - h, 8 * mbh - ch
    margin = padded - interior
    reads = mrows_y * w + 2 * mrows_c * cw + (h if w < 16 * mbw else 0) + (2 * ch if cw < 8 * mbw else 0)
    return {"copy": copy, "in_place": n * (margin + reads), "import_rgba": n * (4 * w * h + padded), "padded": n * padded,
            "margin": n * margin}


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    frame = synth.blobs_rgba(W, H, seed=5, alpha=False)
    rgba = torch.from_numpy(frame).cuda().unsqueeze(0).repeat(N, 1, 1, 1).contiguous()
    for k in range(N):  # distinct frames
        rgba[k, :, :, 0] += k
    mbw, mbh = frames.mb_dims(W, H)
    cw, ch = (W + 1) // 2, (H + 1) // 2
    planes = (torch.empty((N, 16 * mbh, 16 * mbw), dtype=torch.uint8, device="cuda"),
              torch.empty((N, 8 * mbh, 8 * mbw), dtype=torch.uint8, device="cuda"),
              torch.empty((N, 8 * mbh, 8 * mbw), dtype=torch.uint8, device="cuda"))
    work = torch.empty(frames.lib.wg_sharpyuv_work_bytes(W, H, N), dtype=torch.uint8, device="cuda")
    b = moved_bytes(W, H, N)
    out = {}

    def stage(name, fn, nbytes=None):
        med, lo, hi = timed(fn)
        out[name] = {"ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
        if nbytes is not None:
            out[name].update({"bytes": int(nbytes), "GB/s": round(nbytes / med / 1e6, 1)})

    stage("sharpyuv_import_rgba", lambda: frames.sharpyuv_import_rgba(rgba, out=planes, work=work))
    views = (planes[0][:, :H, :W], planes[1][:, :ch, :cw], planes[2][:, :ch, :cw])
    stage("margin_in_place", lambda: frames.import_ycbcr(*views, out=planes), b["in_place"])
    src = tuple(v.contiguous() for v in views)
    dst = tuple(torch.empty_like(p) for p in planes)
    stage("import_ycbcr_copy", lambda: frames.import_ycbcr(*src, out=dst), b["copy"])
    torch.cuda.synchronize()
    assert all(bool((d == p).all()) for d, p in zip(dst, planes)), "copy mode and in place disagree"
    stage("import_rgba", lambda: frames.import_rgba(rgba, has_alpha=False, out=dst), b["import_rgba"])
    print(json.dumps({"config": f"{N} x {W}x{H} RGBA frames (blobs), 1 GPU, {REPS} reps after 3 warm-up calls",
                      "padded_plane_bytes": b["padded"], "margin_bytes": b["margin"], "stages": out}))


if __name__ == "__main__":
    main()
