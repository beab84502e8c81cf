"""Eval metrics of the reference test loop (reference src/ts_hear_test.py:140-146), restated on torch tensors
so they run on the device that holds the separator output (no `outputs.cpu()` round trip).

`scale_invariant_signal_noise_ratio` (torchmetrics, absent here) = zero-mean SI-SDR:
    alpha = (<p,t> + eps) / (<t,t> + eps);  10 log10((|alpha t|^2 + eps) / (|alpha t - p|^2 + eps)), eps = fp32 eps.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def si_snr(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Zero-mean SI-SDR over the last axis, in `pred`'s dtype.  As in torchmetrics, eps follows that dtype: 1.19e-7 on
    float32 inputs — the value the reference's eval and lh_metric_sums use — but 2.2e-16 on float64 ones.  The two differ
    wherever eps decides the result (a silent or constant signal), so this function on doubles is NOT the float64 statement
    of the fp32 metric; tests/data_stage_cases.py restates that with eps fixed at the fp32 value."""
    eps = torch.finfo(pred.dtype).eps
    pred = pred - pred.mean(-1, keepdim=True)
    target = target - target.mean(-1, keepdim=True)
    alpha = ((pred * target).sum(-1, keepdim=True) + eps) / ((target * target).sum(-1, keepdim=True) + eps)
    scaled = alpha * target
    noise = scaled - pred
    return 10.0 * torch.log10(((scaled * scaled).sum(-1) + eps) / ((noise * noise).sum(-1) + eps))


def per_utterance(outputs, mixture, target, embedding, embedding_gt):
    """Rows of the reference CSV (ts_hear_test.py:149-151): output_sisnr, si_snr_i, embedding_sim — each [B]."""
    out_sisnr = si_snr(outputs, target)                                   # [B, 2]
    snr_i = out_sisnr - si_snr(mixture, target)
    return (out_sisnr.mean(dim=1), snr_i.reshape(snr_i.shape[0], -1).mean(dim=1),
            F.cosine_similarity(embedding, embedding_gt, dim=-1))


def metric_sums(outputs, mixture, target, embedding, embedding_gt) -> torch.Tensor:
    """[sum si_snr_i, sum output_sisnr, sum embedding_sim, n] as fp64 on the outputs' device — the 32-byte
    payload of the sharded eval's single all-reduce."""
    o, i, c = per_utterance(outputs, mixture, target, embedding, embedding_gt)
    n = torch.tensor(float(outputs.shape[0]), device=outputs.device, dtype=torch.float64)
    return torch.stack([i.double().sum(), o.double().sum(), c.double().sum(), n])


def metric_sums_device(outputs, mixture, target, embedding, embedding_gt, host=None):
    """Same quantities through the HIP kernels of lh_metrics.hip (fp64 moments, one pass over the waveforms).
    Returns (sums [4] fp64 on device, rows [B,3] fp32 = output_sisnr, si_snr_i, embedding_sim).  `host`: the
    `_cabi.HipHost` whose library / stream plumbing to use (default: the product library on the tensors' GPU)."""
    from . import _cabi
    if host is None:
        host = type("MetricHost", (_cabi.HipHost,), {"_host_name": "metric_sums_device"})()
    lib = host._lib(outputs)
    B, _, n = outputs.shape
    dev = outputs.device
    c32 = lambda t: t.contiguous().float()
    o, m, t = c32(outputs), c32(mixture), c32(target)
    e, g = c32(embedding.reshape(B, -1)), c32(embedding_gt.reshape(B, -1))
    scratch = torch.empty(B * 2 * 16 * 8 + B * 3, dtype=torch.float64, device=dev)
    rows = torch.empty(B, 3, dtype=torch.float32, device=dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    st = host._stream(dev)
    with host._device_ctx(o):
        lib.call("lh_metric_sums", o.data_ptr(), t.data_ptr(), m.data_ptr(), e.data_ptr(), g.data_ptr(),
                 scratch.data_ptr(), rows.data_ptr(), sums.data_ptr(), B, n, e.shape[1], st)
    return sums, rows


# ---- binaural cue errors (reference src/eval/binaural.py: itd_diff, ild_diff, chunk_and_mask) --------------------------------
BINAURAL_TMAX = 16              # largest round(1e-3 sr) lh_binaural_cues is compiled for (sr <= 16500)
BINAURAL_RMS_THRESHOLD = 1e-3   # chunk_and_mask's rms_threshold
_SEG_FIELDS = ("tau_est", "tau_gt", "ild_est", "ild_gt", "itd_est", "itd_gt", "counted")


def binaural_lengths(n_samples: int, sr: int, moving: bool):
    """(t_max, frame) of the reference for a clip of `n_samples` at `sr`: t_max = round(1e-3 sr) lags each side,
    frame = round(0.25 sr) samples in moving mode, 0 in static mode.  Raises ValueError for what the restatement and the
    kernel do not define: an odd clip in static mode (the reference's irfft then returns n - 1 points, another quantity),
    an odd frame, and t_max outside 1 .. BINAURAL_TMAX."""
    t_max = int(round(1e-3 * sr))
    if not 1 <= t_max <= BINAURAL_TMAX:
        raise ValueError(f"binaural cues: sr {sr} gives t_max {t_max}; supported 1 .. {BINAURAL_TMAX} (sr 500 .. 16500)")
    if not moving:
        if n_samples % 2:
            raise ValueError(f"binaural cues: static mode needs an even clip length, got {n_samples}")
        return t_max, 0
    frame = int(round(1e-3 * 250 * sr))
    if frame % 2:
        raise ValueError(f"binaural cues: moving mode needs an even frame round(0.25 sr), got {frame} at sr {sr}")
    return t_max, frame


def _segment_cues(x: torch.Tensor, sr: int, t_max: int):
    """x [..., 2, L] fp64 -> (tau, ild) [...] of compute_itd / compute_ild: the circular cross-correlation by FFT, as the
    reference computes it, argmax |cc| over lags -t .. t (first maximum wins), t = min(t_max, L // 2)."""
    L = x.shape[-1]
    left, right = x[..., 0, :], x[..., 1, :]
    ild = 10.0 * torch.log10((left * left).sum(-1) / (right * right).sum(-1))
    corr = torch.fft.irfft(torch.fft.rfft(left) * torch.fft.rfft(right).conj(), n=L)
    t = min(t_max, L // 2)
    cc = torch.cat([corr[..., L - t:], corr[..., :t + 1]], dim=-1)
    tau = torch.argmax(cc.abs(), dim=-1).double() - t
    return tau, ild


def binaural_errors(est: torch.Tensor, gt: torch.Tensor, sr: int = 16000, moving: bool = False,
                    return_segments: bool = False):
    """Per-utterance binaural cue errors of the reference's `itd_diff` / `ild_diff` (src/eval/binaural.py), restated in
    torch fp64 on host tensors.  est, gt [B, 2, N] (channel 0 = left, 1 = right).  Returns rows [B, 2] fp64 =
    (delta_itd_us, delta_ild_db); with `return_segments` also a dict of [B, C] tensors (tau_est, tau_gt, ild_est, ild_gt,
    itd_est, itd_gt, counted).

    Per segment: ILD = 10 log10(sum L^2 / sum R^2) and ITD = tau / sr * 1e6 us with tau = argmax |cc| of the circular
    cross-correlation over lags -round(1e-3 sr) .. +round(1e-3 sr).  Static mode: one segment, the whole clip;
    |ITD_est - ITD_gt| and |ILD_est - ILD_gt|.  Moving mode (chunk_and_mask): frames of round(0.25 sr) samples, the last
    one zero-padded, counted when the target's RMS over the frame reaches 1e-3 on either channel; the mean over counted
    frames of |ITD_est - ITD_gt|, and |mean ILD_est - mean ILD_gt| (means first); NaN when no frame counts.  Silent
    channels give inf / NaN by IEEE rules.

    The definition held to is the reference's result on FLOAT64 copies of the inputs (fed float32 arrays, the reference
    itself works in single precision: scipy's rfft keeps float32).  Lengths it refuses: `binaural_lengths`."""
    B, _, n = est.shape
    t_max, frame = binaural_lengths(n, sr, moving)
    e, g = est.detach().cpu().double(), gt.detach().cpu().double()
    if moving:
        C = -(-n // frame)
        pad = C * frame - n
        e = torch.nn.functional.pad(e, (0, pad)).reshape(B, 2, C, frame).transpose(1, 2)      # [B, C, 2, FW]
        g = torch.nn.functional.pad(g, (0, pad)).reshape(B, 2, C, frame).transpose(1, 2)
        counted = (g * g).mean(-1).sqrt().amax(-1) >= BINAURAL_RMS_THRESHOLD                    # [B, C]
    else:
        e, g = e[:, None], g[:, None]
        counted = torch.ones(B, 1, dtype=torch.bool)
    tau_e, ild_e = _segment_cues(e, sr, t_max)
    tau_g, ild_g = _segment_cues(g, sr, t_max)
    itd_e, itd_g = tau_e / sr * 1e6, tau_g / sr * 1e6
    cnt = counted.double().sum(1)
    zero = torch.zeros((), dtype=torch.float64)
    d_itd = torch.where(counted, (itd_e - itd_g).abs(), zero).sum(1) / cnt
    d_ild = (torch.where(counted, ild_e, zero).sum(1) / cnt - torch.where(counted, ild_g, zero).sum(1) / cnt).abs()
    rows = torch.stack([d_itd, d_ild], dim=1)
    if not return_segments:
        return rows
    segs = dict(zip(_SEG_FIELDS, (tau_e, tau_g, ild_e, ild_g, itd_e, itd_g, counted)))
    return rows, segs


def binaural_sums(rows: torch.Tensor) -> torch.Tensor:
    """[sum delta_itd over finite rows, count, sum delta_ild over finite rows, count] fp64 from rows [B, 2] — what
    lh_binaural_cues writes as `sums`, for the host path of the sharded eval."""
    fin = torch.isfinite(rows)
    s = torch.where(fin, rows, torch.zeros((), dtype=rows.dtype, device=rows.device)).double().sum(0)
    c = fin.double().sum(0)
    return torch.stack([s[0], c[0], s[1], c[1]])


def binaural_errors_device(est, gt, sr: int = 16000, moving: bool = False, host=None, return_segments: bool = False):
    """`binaural_errors` through the HIP kernels of lh_metrics.hip (direct fp64 lag sums, no FFT).  Returns (sums [4] fp64,
    rows [B, 2] fp64) on the device: sums as `binaural_sums`, rows = (delta_itd_us, delta_ild_db); with `return_segments`
    also the segment records, a dict of [B, C] tensors as `binaural_errors` gives.  `host`: as in `metric_sums_device`."""
    from . import _cabi
    if host is None:
        host = type("MetricHost", (_cabi.HipHost,), {"_host_name": "binaural_errors_device"})()
    B, _, n = est.shape
    t_max, frame = binaural_lengths(n, sr, moving)
    lib = host._lib(est)
    seglen = frame if moving else n
    C = -(-n // frame) if moving else 1
    tiles = -(-seglen // 4096)
    dev = est.device
    e, g = est.contiguous().float(), gt.contiguous().float()
    scratch = torch.empty(B * C * (tiles * 72 + 8), dtype=torch.float64, device=dev)
    rows = torch.empty(B, 2, dtype=torch.float64, device=dev)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    st = host._stream(dev)
    with host._device_ctx(e):
        lib.call("lh_binaural_cues", e.data_ptr(), g.data_ptr(), scratch.data_ptr(), rows.data_ptr(), sums.data_ptr(),
                 B, n, int(sr), frame, BINAURAL_RMS_THRESHOLD, st)
    if not return_segments:
        return sums, rows
    rec = scratch[B * C * tiles * 72:].view(B, C, 8)
    segs = {k: rec[..., i] for i, k in enumerate(_SEG_FIELDS)}
    segs["counted"] = segs["counted"] != 0
    return sums, rows, segs
