"""Phase B on one GPU over the bench's own batch: N x 1920x1080 frames, contents
gradient / noise / photo in turn with seed = frame index (bench.py's
frame_rgba), encoded by frames.encode_frames with the default configuration.
Measures, with HIP events on the current stream after a warm-up (median of
REPS, min and max beside it):

  token_stats    wg_encode_token_stats: clear + k_tok_mbctx + k_tok_dcwalk +
                 k_tok_count + k_tok_scan + k_tok_proba
  tokens         wg_encode_tokens: k_tok_write
  d2h_mb_enc     the wg_mb_enc records to pinned host memory (what a host
                 Phase B needs: 864 B / MB)
  d2h_phase_b    hdr + each image's tokens (+ probabilities and summaries) to
                 pinned memory, one copy per image for the tokens

with the bytes each moves computed from the shapes and the token totals, and
the fraction of the 8.0 TB/s HBM peak; tokens per MB of the mix; the host time
of wg_vp8_emit per frame; and, for the first frame of each content, the serial
restatement's token count (tests/phase_b.py), compared with the device's
tokens byte for byte.  The per-kernel split of token_stats comes from a
profiler run of this script with KERNELS_ONLY=1 (no copies, no host work).
No threshold: prints one JSON line.  Environment: N, REPS, KERNELS_ONLY."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools import synth  # noqa: E402
from webp_amd import frames  # noqa: E402

N = int(os.environ.get("N", "64"))
REPS = int(os.environ.get("REPS", "20"))
KERNELS_ONLY = os.environ.get("KERNELS_ONLY", "0") == "1"
W, H = 1920, 1080
CONTENTS = ("grad", "noise", "photo")
HBM_PEAK_GBS = 8000.0  # MI355X: 8.0 TB/s spec, as bench.py


def frame_rgba(g):
    kind = CONTENTS[g % 3]
    return {"grad": synth.gradient_rgba, "noise": synth.noise_rgba, "photo": synth.photo_rgba}[kind](W, H, seed=g)


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


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    mbw, mbh = frames.mb_dims(W, H)
    nmb = mbw * mbh
    rgba = torch.empty((N, H, W, 4), dtype=torch.uint8, device=dev)
    for i in range(N):
        rgba[i].copy_(torch.from_numpy(frame_rgba(i)))
    cfg = frames.encoder_config()
    mb_enc, _, _, _, info = frames.encode_frames(rgba, cfg=cfg)
    del rgba
    hdr, proba_out, summ, tokens, stats = frames.encode_tokens(mb_enc, mbw, mbh)
    torch.cuda.synchronize()
    totals = summ["total_tokens"].astype(np.int64)
    pitch = tokens.shape[1]
    work = torch.empty(frames.lib.wg_encode_tokens_work_bytes(mbw, mbh, N), dtype=torch.uint8, device=dev)
    summary = torch.empty((N, 16), dtype=torch.uint8, device=dev)
    proba_in = frames.default_proba(dev)
    s = torch.cuda.current_stream().cuda_stream

    def run_stats():
        frames.call("wg_encode_token_stats", mb_enc.data_ptr(), mbw, mbh, N, proba_in.data_ptr(), 0, stats.data_ptr(),
                    proba_out.data_ptr(), hdr.data_ptr(), summary.data_ptr(), work.data_ptr(), s)

    def run_tokens():
        frames.call("wg_encode_tokens", mb_enc.data_ptr(), mbw, mbh, N, proba_out.data_ptr(), hdr.data_ptr(),
                    work.data_ptr(), tokens.data_ptr(), pitch, s)

    out = {}

    def stage(name, fn, nbytes):
        med, lo, hi = timed(fn)
        out[name] = {"ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "bytes": int(nbytes),
                     "GB/s": round(nbytes / med / 1e6, 1), "hbm_frac": round(nbytes / med / 1e6 / HBM_PEAK_GBS, 4)}

    rec_bytes = N * nmb * 864
    tok_bytes = int(2 * totals.sum())
    # token_stats: k_tok_mbctx reads the 64-byte tail of every record and writes 24 B of hdr + a 4 B context word;
    # k_tok_dcwalk reads the words twice and writes 2 B / MB; k_tok_count reads every record once plus its two
    # neighbours' words and writes tok_count; the scan reads and writes 8 B of hdr per MB
    stats_bytes = N * nmb * (64 + 28 + 8 + 2 + 864 + 12 + 4 + 16) + N * (2112 * 4 * 2 + 1056 * 2)
    stage("token_stats", run_stats, stats_bytes)
    # tokens: every record read once, the tokens written once, hdr (8 B) and context (10 B) read per MB
    stage("tokens", run_tokens, rec_bytes + tok_bytes + N * nmb * 18)
    result = {"config": f"{N} x {W}x{H} frames (gradient / noise / photo in turn), default encoder configuration, 1 GPU, "
                        f"{REPS} reps after 3 warm-up calls",
              "macroblocks": N * nmb, "tokens_total": int(totals.sum()),
              "tokens_per_mb": {"all": round(float(totals.sum()) / (N * nmb), 2),
                                **{k: round(float(totals[i::3].mean()) / nmb, 2) for i, k in enumerate(CONTENTS) if i < N}},
              "skipped_mbs": int(summ["num_skip"].sum()), "proba_updates_per_frame": round(float(summ["num_updates"].mean()), 1),
              "stages": out}
    if KERNELS_ONLY:
        print(json.dumps(result))
        return
    # the two device-to-host copies, to pinned memory
    host_rec = torch.empty(mb_enc.shape, dtype=torch.uint8).pin_memory()
    host_hdr = torch.empty(hdr.shape, dtype=torch.uint8).pin_memory()
    # tokens: each image's own range (2 * total_tokens bytes), packed back to back
    tok_off = np.concatenate([[0], np.cumsum(2 * totals)]).astype(np.int64)
    host_tok = torch.empty(int(tok_off[-1]), dtype=torch.uint8).pin_memory()
    host_proba = torch.empty(proba_out.shape, dtype=torch.uint8).pin_memory()
    host_sum = torch.empty(summary.shape, dtype=torch.uint8).pin_memory()

    def copy_b():
        host_hdr.copy_(hdr, non_blocking=True)
        for i in range(N):
            host_tok[tok_off[i]:tok_off[i + 1]].copy_(tokens[i, :2 * int(totals[i])], non_blocking=True)
        host_proba.copy_(proba_out, non_blocking=True)
        host_sum.copy_(summary, non_blocking=True)

    stage("d2h_mb_enc", lambda: host_rec.copy_(mb_enc, non_blocking=True), rec_bytes)
    b_bytes = hdr.numel() + tok_bytes + proba_out.numel() + summary.numel()
    stage("d2h_phase_b", copy_b, b_bytes)
    for k in ("d2h_mb_enc", "d2h_phase_b"):
        out[k].pop("hbm_frac")
    result["d2h_bytes_per_mb"] = {"mb_enc": 864, "phase_b": round(b_bytes / (N * nmb), 1), "hdr": 32,
                                  "tokens": {"all": round(tok_bytes / (N * nmb), 1),
                                             **{k: round(2 * float(totals[i::3].mean()) / nmb, 1)
                                                for i, k in enumerate(CONTENTS) if i < N}}}
    # host: wg_vp8_emit per frame, and the serial restatement on the first frame of each content
    torch.cuda.synchronize()
    hdr_h, proba_h = host_hdr.numpy(), host_proba.numpy()
    tok_h = [host_tok.numpy()[tok_off[i]:tok_off[i + 1]] for i in range(N)]
    info_h = info.cpu().numpy()
    emit_ms, sizes = [], []
    for i in range(N):
        t0 = time.perf_counter()
        data = frames.vp8_emit(W, H, cfg, info_h[i], hdr_h[i], proba_h[i], summ[i:i + 1], tok_h[i])
        emit_ms.append(1e3 * (time.perf_counter() - t0))
        sizes.append(len(data))
    result["vp8_emit_host"] = {"ms_per_frame_median": round(float(np.median(emit_ms)), 2),
                               "ms_per_frame_max": round(float(max(emit_ms)), 2),
                               "file_bytes_mean": int(np.mean(sizes)), "note": "one thread, includes the ctypes wrapper"}
    import phase_b as PB
    serial = {}
    rec_h = host_rec.numpy().view(PB.MB_ENC_DTYPE).reshape(N, nmb)
    for i, k in enumerate(CONTENTS[:N]):
        t0 = time.perf_counter()
        pb = PB.phase_b(rec_h[i], mbw, mbh)
        same = (pb["tokens"].size == 2 * int(totals[i]) and bool((tok_h[i][:pb["tokens"].size] == pb["tokens"]).all())
                and hdr_h[i].tobytes() == pb["hdr"].tobytes() and bool((proba_h[i] == pb["proba"]).all()))
        serial[k] = {"tokens": int(pb["tokens"].size // 2), "device_tokens": int(totals[i]), "identical": same,
                     "python_s": round(time.perf_counter() - t0, 1)}
    result["serial_restatement"] = serial
    print(json.dumps(result))


if __name__ == "__main__":
    main()
