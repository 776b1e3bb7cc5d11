"""Host-side checks of the front-end and resampler index arithmetic (no GPU): numpy restatements of what
csrc/logmel.hip and csrc/resample.hip compute for addresses, checked against numpy / torch and against coverage rules."""
import math

import numpy as np
import pytest

# ------------------------------------------------------------------------------------------------ log-mel framing
# Cfg<KIND> of csrc/logmel.hip: (WIN = K, HOP, NFFT, CENTER)
CFG = {"vggish": (400, 160, 512, 0), "whisper": (400, 160, 400, 1), "htsat": (1024, 480, 1024, 1)}
FT = 32                                                          # frames per workgroup


def kernel_frame_indices(n: int, kind: str, n_frames: int) -> np.ndarray:
    """-> [n_frames, K] sample index each frame's DFT reads, -1 for a zero, as logmel_kernel stages and reads them:
    per workgroup the span p0 + s (s < SPAN) is reflected ONCE (p < 0 -> -p, then p >= L -> 2(L-1) - p), stored at the
    skewed slot s + 2 (s / HOP), and frame i of the workgroup reads slot i (HOP + 2) + k + 2 (k / HOP)."""
    K, HOP, NFFT, CENTER = CFG[kind]
    SPAN = (FT - 1) * HOP + K
    SPAN_SK = SPAN + 2 * (SPAN // HOP) + 2
    L = n
    out = np.empty((n_frames, K), np.int64)
    s = np.arange(SPAN)
    k = np.arange(K)
    for f0 in range(0, n_frames, FT):
        p = f0 * HOP - (NFFT // 2 if CENTER else 0) + s
        if CENTER:
            p = np.where(p < 0, -p, p)
            p = np.where(p >= L, 2 * (L - 1) - p, p)
        v = np.where((p >= 0) & (p < L), p, -1)
        xs = np.full(SPAN_SK, -7, np.int64)                      # -7: a slot nothing was stored to
        xs[s + 2 * (s // HOP)] = v
        for i in range(min(FT, n_frames - f0)):
            out[f0 + i] = xs[i * (HOP + 2) + k + 2 * (k // HOP)]
    assert (out != -7).all()
    return out


def test_torch_stft_reflect_rule_behind_the_htsat_refusal():
    """The reference's HTSAT front end is torch.stft(center=True, pad_mode="reflect") with n_fft 1024: the pad (512) must be
    shorter than the clip.  fad_logmel_htsat refuses the same clips (<= 512 samples) instead of returning a frame no reference
    can produce."""
    import torch
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64)

    def stft(n):
        return torch.stft(torch.linspace(-1, 1, n, dtype=torch.float64), n_fft=1024, hop_length=480, win_length=1024,
                          window=win, center=True, pad_mode="reflect", return_complex=True)
    for n in (2, 300, 512):
        with pytest.raises(RuntimeError):
            stft(n)
    assert stft(513).shape == (513, 2)


def test_kernel_reflect_map_equals_numpy_pad_above_512():
    """One reflection is numpy's (and torch's) reflect padding exactly when the pad is shorter than the clip: for every HTSAT
    clip length 513 .. 3000 and every frame, the kernel's index map equals np.pad(mode="reflect"); at 512 and below it does not
    for many (2 .. 496: 272 of them), and torch refuses all of them, which is why the library refuses clips of <= 512 samples."""
    for n in range(513, 3001):
        nfr = 1 + n // 480
        want = np.pad(np.arange(n), 512, mode="reflect")[480 * np.arange(nfr)[:, None] + np.arange(1024)[None, :]]
        got = kernel_frame_indices(n, "htsat", nfr)
        if not np.array_equal(got, want):
            raise AssertionError(f"n={n}: kernel reflect map differs from np.pad in {(got != want).sum()} places")
    for n in (2, 100, 256, 496):
        nfr = 1 + n // 480
        want = np.pad(np.arange(n), 512, mode="reflect")[480 * np.arange(nfr)[:, None] + np.arange(1024)[None, :]]
        assert not np.array_equal(kernel_frame_indices(n, "htsat", nfr), want), n


@pytest.mark.parametrize("kind", ["vggish", "whisper"])
def test_kernel_frame_map_16k_front_ends(kind):
    """VGGish frames are x[160 f + k] (no padding, frames only where the clip covers them); Whisper pads / cuts to 480 000
    samples (zeros) and reflects 200 samples at each end, like np.pad(reflect) on the padded signal.  Across workgroup edges
    (32 frames) the skewed LDS slots give every frame its own samples."""
    if kind == "vggish":
        for n in (400, 15600, 15600 + 15360 + 1):
            nfr = 1 + (n - 400) // 160
            want = 160 * np.arange(nfr)[:, None] + np.arange(400)[None, :]
            assert np.array_equal(kernel_frame_indices(n, kind, nfr), want)
    else:
        L = 480000
        got = kernel_frame_indices(L, kind, 3000)
        want = np.pad(np.arange(L), 200, mode="reflect")[160 * np.arange(3000)[:, None] + np.arange(400)[None, :]]
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ resampler launch shape
MAX_SPAN = 16384


def resample_launch(orig_sr: int, new_sr: int, n: int) -> dict:
    """The launch arithmetic of fad_resample_kaiser (csrc/resample.hip), restated."""
    g = math.gcd(orig_sr, new_sr)
    orig, nnew = orig_sr // g, new_sr // g
    base = min(orig, nnew) * 0.9475937167399596
    width = math.ceil(64.0 * orig / base)
    taps = 2 * width + orig
    frames = n // orig + 1
    n_out = (nnew * n + orig - 1) // orig
    gy = -(-nnew // 256)
    fb8 = 7 * orig + taps <= MAX_SPAN
    fb = 8 if fb8 else 1
    groups = 256 // nnew if nnew < 256 else 1
    by_lds = (MAX_SPAN - taps + orig) // (fb * orig)
    groups = max(1, min(groups, by_lds))
    span = (groups * fb - 1) * orig + taps
    gx = -(-frames // (groups * fb))
    return dict(orig=orig, nnew=nnew, width=width, taps=taps, frames=frames, n_out=n_out, gy=gy, fb=fb, groups=groups,
                by_lds=by_lds, span=span, gx=gx)


def resample_writes(s: dict) -> np.ndarray:
    """-> how often resample_kernel writes each output index 0 .. n_out - 1 under the launch `s` (thread -> (group, phase))."""
    tid = np.arange(256)
    per = min(s["nnew"], 256)
    grp, ph = tid // per, tid % per
    bx = np.arange(s["gx"])[:, None, None, None]
    by = np.arange(s["gy"])[None, :, None, None]
    fr = np.arange(s["fb"])[None, None, None, :]
    p = by * 256 + ph[None, None, :, None]
    f = bx * s["groups"] * s["fb"] + grp[None, None, :, None] * s["fb"] + fr
    o = f * s["nnew"] + p
    live = (grp[None, None, :, None] < s["groups"]) & (p < s["nnew"]) & (f < s["frames"]) & (o < s["n_out"])
    o, live = np.broadcast_arrays(o, live)
    return np.bincount(o[live].ravel(), minlength=s["n_out"])


PAIRS = [(16000, 44100), (22050, 48000), (11025, 48000), (44056, 16000), (96000, 16000), (48000, 16000),
         (44100, 16000), (8000, 16000), (22050, 24000), (44100, 48000), (32000, 48000)]


@pytest.mark.parametrize("orig_sr,new_sr", PAIRS)
def test_resampler_launch_covers_every_output_once(orig_sr, new_sr):
    """For each rate pair and the lengths the GPU tests use (1, orig - 1, orig, orig + 1, a ragged last workgroup, a long
    signal): the LDS span stays within 64 KiB, every read of the span stays inside it, and every output (frame, phase) is
    written by exactly one thread."""
    s0 = resample_launch(orig_sr, new_sr, 1)
    orig = s0["orig"]
    wg = s0["groups"] * s0["fb"] * orig                        # input samples per workgroup
    for n in (1, orig - 1, orig, orig + 1, 3 * wg + 7 * orig // 3 + 1, 60 * orig_sr + 12345):
        if n < 1:
            continue
        s = resample_launch(orig_sr, new_sr, n)
        assert s["span"] <= MAX_SPAN and s["by_lds"] >= 1, s
        assert (s["groups"] * s["fb"] - 1) * orig + s["taps"] - 1 < s["span"]         # last tap of the last frame group
        assert s["gy"] * 256 >= s["nnew"] and s["gx"] * s["groups"] * s["fb"] >= s["frames"]
        assert s["frames"] * s["nnew"] >= s["n_out"]
        w = resample_writes(s)
        assert w.shape == (s["n_out"],) and (w == 1).all(), (n, np.flatnonzero(w != 1)[:8], s)


def test_resampler_launch_shapes_of_the_edge_pairs():
    """The pairs the GPU edge tests were chosen for take the branches they are meant to: more than 256 phases (blockIdx.y
    tiles), FB = 1 (7 orig + taps > 16 384), and many frame groups per workgroup."""
    assert [resample_launch(o, n, 1)["gy"] for o, n in ((16000, 44100), (22050, 48000), (11025, 48000))] == [2, 2, 3]
    s = resample_launch(44056, 16000, 1)
    assert (s["orig"], s["nnew"], s["taps"], s["fb"], s["gy"]) == (5507, 2000, 5879, 1, 8)
    assert resample_launch(96000, 16000, 1)["groups"] == 256 and resample_launch(48000, 16000, 1)["groups"] == 256
