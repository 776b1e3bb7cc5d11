"""Log-mel front ends (csrc/logmel.hip) and the resampler (csrc/resample.hip) at their edges, against the float64 oracles.

Every tolerance is a per-element bound derived from the kernels' arithmetic and evaluated on the float64 reference
(u = 2^-24, the fp32 unit roundoff):

DFT.  Frame f holds samples x_{f,k}, k < K, with the window w_k folded into fp32 cos / sin tables (each entry off by at most
u relative).  The MFMA (exact fp32 products) adds 4 products per step into an fp32 accumulator over K/4 steps, so each of
Re X_b and Im X_b is off by at most eps_f = (K/4 + 5) u S_f,  S_f = sum_k |x_{f,k} w_k|  (table rounding, the rounded sums
of 4, and one rounding per step, first order).
Power (Whisper, HTSAT).  P = Re^2 + Im^2:  |dP| <= 2 (|Re| + |Im|) eps + 2 eps^2 + 3 u P <= 2 sqrt(2P) eps + 2 eps^2 + 3 u P,
plus 2^-126 for a result flushed to zero.
Magnitude (VGGish).  |X| is 1-Lipschitz in (Re, Im):  |dA| <= sqrt(2) eps + 2.5 u (A + sqrt(2) eps) + 2^-63 (the sqrt of a
flushed square).
Mel.  M_m = sum_b W_bm F_b with W >= 0 (fp32 table) accumulated over bins_pad / 4 MFMA steps:
    E_m = sum_b W_bm dF_b + (bins_pad / 4 + 5) u sum_b W_bm (F_b + dF_b).
Log.  A device log is a few ulp: 4 u (|y| + 1) covers log2-based implementations near y = 0.
  VGGish   y = log(M + 0.01):  |dy| <= D / (M + 0.01 - D) + 4 u (|y| + 1),  D = E + 2 u (M + 0.01)  (0.01f and the add).
  HTSAT    z = 10 log10(max(M, 1e-10)).  Well above the floor (M - E > 1e-9):  |dz| <= 10 log10(e) E / (M - E) + rounding.
           Near the floor the check is linear:  |max(10^(z'/10), 1e-10) - max(M, 1e-10)| <= E (1 + rel) + r rel + u 1e-10,
           r = max(M, 1e-10), rel = 10^(rounding / 10) - 1.
  Whisper  v = log10(max(M, 1e-10)), out = (max(v, vmax - 8) + 4) / 4.  Bv = log10(e) E / max(M - E, 1e-10) + rounding.
           The clip maximum moves by at most Bm = max{Bv_j : v_j + Bv_j >= vmax - Bv_argmax} (1-Lipschitz max).  Elements
           a decade above both the floor and the clamp (M - E > 10 max(1e-10, 10^(vmax - 8 + Bm))) are checked in the log
           domain, |d out| <= Bv / 4 + 2 u (|out| + 3); the rest in the linear domain, g = 10^(4 out' - 4) against
           r = max(M, 1e-10, 10^(vmax - 8)):  |g - r| <= E (1 + rel) + r rel + u 1e-10,  rel = 10^(max(Bm, dlog) + 4 rnd) - 1.
Resampler.  out = sum_j K_j x_j by sequential fmaf over the taps.  Each fma rounds once, at most u |s_j| for the running
  sum s_j, so (running error bound, first order) |d out| <= 1.001 u (sum_j |s_j| + sum_j |K_j x_j|), the second term for
  a table entry rounded to the other fp32 neighbour.  The partial sums come from the float64 reference.  PCM16: where the
  float64 value is farther than that bound from a rounding boundary the quantised sample is exact, else within 1 LSB.

Where a case repeats a signal family, length and rate pair that tests/test_frontend.py or tests/test_gpu_pipeline.py
already cover (recipes.audio_clip), the old fixed tolerance is asserted as well, so no check is looser than before.
Each case prints one `[fe-err]` line: the largest error and the largest error / bound ratio.
"""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import recipes as R
from oracle import audio_oracle as AO
from oracle import logmel_oracle as L

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LOG10E = math.log10(math.e)
FE = {"vggish": dict(K=400, hop=160, nfft=512, bins_pad=272),      # Cfg<KIND> of csrc/logmel.hip, bins padded to 16
      "whisper": dict(K=400, hop=160, nfft=400, bins_pad=208),
      "htsat": dict(K=1024, hop=480, nfft=1024, bins_pad=528)}
SPLIT = 32768                                                      # clips per launch (gridDim.y)


# ------------------------------------------------------------------------------------------------ references and bounds
def _frames64(kind, x):
    x = np.asarray(x, np.float32).astype(np.float64)
    if kind == "vggish":
        n_ex = L.vggish_num_examples(len(x))
        return L._frames(x, 400, 160)[:n_ex * 96] if n_ex else np.zeros((0, 400))
    if kind == "whisper":
        x = np.pad(x[:480000], (0, max(0, 480000 - len(x))))
        return L._frames(np.pad(x, 200, mode="reflect"), 400, 160)[:3000]
    return L._frames(np.pad(x, 512, mode="reflect"), 1024, 480)


def mel_with_bound(kind, x, n_mels=64):
    """-> (M, E): float64 mel energies [frames, n_mels] the kernel forms before its log, and the bound on its error."""
    c = FE[kind]
    xw = _frames64(kind, x) * L._periodic_hann(c["K"])
    X = np.fft.rfft(xw, c["nfft"], axis=1)
    eps = (c["K"] / 4 + 5) * U * np.abs(xw).sum(1, keepdims=True)
    if kind == "vggish":
        F = np.abs(X)
        dF = math.sqrt(2) * eps + 2.5 * U * (F + math.sqrt(2) * eps) + 2.0 ** -63
        W = L.mel_htk_vggish()
    else:
        F = X.real ** 2 + X.imag ** 2
        dF = 2 * np.sqrt(2 * F) * eps + 2 * eps ** 2 + 3 * U * F + 2.0 ** -126
        W = L.mel_slaney(201, n_mels, 16000.0, 0.0, 8000.0) if kind == "whisper" else L.mel_slaney(513, 64, 48000.0, 50.0, 14000.0)
    M = F @ W
    return M, dF @ W + (c["bins_pad"] / 4 + 5) * U * ((F + dF) @ W)


def _judge(label, parts, got=None, ref=None, fixed=None):
    """parts: (domain, err, bound) arrays.  Asserts err <= bound everywhere (and |got - ref| <= fixed), prints one line."""
    worst, ratio, desc = 0.0, 0.0, []
    for dom, err, bound in parts:
        if err.size == 0:
            continue
        r = err / bound
        k = int(np.argmax(r))
        desc.append(f"{dom} n={err.size} max|err|={err.max():.3e} max err/bound={r.flat[k]:.3f}")
        worst, ratio = max(worst, float(err.max())), max(ratio, float(r.flat[k]))
        assert (err <= bound).all(), (label, dom, float(err.flat[k]), float(bound.flat[k]), k)
    line = f"[fe-err] {label}: " + "; ".join(desc or ["empty"])
    if fixed is not None and got is not None and got.size:
        d = float(np.abs(got.astype(np.float64) - ref).max())
        line += f"; fixed {fixed:.0e} max|err|={d:.3e}"
        assert d <= fixed, (label, d, fixed)
    print(line)
    return ratio


def check_vggish(got, x, label, fixed=None):
    got = np.asarray(got, np.float64).reshape(-1, 64)
    M, E = mel_with_bound("vggish", x)
    ref = L.vggish_examples(x).reshape(-1, 64)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    np.testing.assert_allclose(np.log(M + 0.01), ref, rtol=0, atol=1e-12)      # the bound is about the oracle's quantity
    A = M + 0.01
    D = E + 2 * U * A
    bound = D / (A - D) + 4 * U * (np.abs(ref) + 1)
    return _judge(label, [("log", np.abs(got - ref), bound)], got, ref, fixed)


def check_htsat(got, x, label, fixed=None):
    got = np.asarray(got, np.float64).reshape(-1, 64)
    M, E = mel_with_bound("htsat", x)
    ref = L.htsat_logmel(x)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    lm = np.log10(np.maximum(M, 1e-10))
    np.testing.assert_allclose(10 * lm, ref, rtol=0, atol=1e-9)
    rnd = 10 * (4 * U * (np.abs(lm) + 1) + U) + U * np.abs(ref)                # log10f, 1e-10f, the product by 10
    far = M - E > 1e-9
    parts = [("log", np.abs(got - ref)[far], (10 * LOG10E * E / np.where(far, M - E, 1.0) + rnd)[far])]
    r = np.maximum(M, 1e-10)
    rel = 10 ** (rnd / 10) - 1
    g = np.maximum(10 ** (got / 10), 1e-10)
    parts.append(("linear", np.abs(g - r)[~far], (E * (1 + rel) + r * rel + U * 1e-10)[~far] * (1 + 1e-9)))
    return _judge(label, parts, got, ref, fixed)


def check_whisper(got, x, n_mels, label, fixed=None):
    got = np.asarray(got, np.float64)
    M, E = mel_with_bound("whisper", x, n_mels)                   # [3000, n_mels]
    ref = L.whisper_features(x, n_mels)                           # [n_mels, 3000]
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    v = np.log10(np.maximum(M, 1e-10))
    vmax = v.max()
    np.testing.assert_allclose(((np.maximum(v, vmax - 8) + 4) / 4).T, ref, rtol=0, atol=1e-12)
    dlog = 4 * U * (np.abs(v) + 1) + U
    Bv = LOG10E * E / np.maximum(M - E, 1e-10) + dlog
    Bm = Bv[v + Bv >= vmax - Bv.flat[int(np.argmax(v))]].max()
    rnd = 2 * U * (np.abs(ref.T) + 3)
    far = M - E > 10 * max(1e-10, 10 ** (vmax - 8 + Bm))
    g_err = np.abs(got.T - ref.T)
    parts = [("log", g_err[far], (Bv / 4 + rnd)[far])]
    r = np.maximum(np.maximum(M, 1e-10), 10 ** (vmax - 8))
    rel = 10 ** (np.maximum(Bm, dlog) + 4 * rnd) - 1
    g = 10 ** (4 * got.T - 4)
    parts.append(("linear", np.abs(g - r)[~far], (E * (1 + rel) + r * rel + U * 1e-10)[~far] * (1 + 1e-9)))
    return _judge(label, parts, got, ref, fixed)


def resample_ref_bound(x, orig_sr, new_sr, fa, fb):
    """Output frames [fa, fb) (frame f = outputs f*new .. f*new + new - 1) of the float64 convolution, and the running-error
    bound of the kernel's sequential fp32 fma over the taps."""
    k, width, orig, new = AO.sinc_kernel(orig_sr, new_sr)
    k = k.astype(np.float64)
    taps, n = k.shape[1], len(x)
    x64 = np.asarray(x, np.float32).astype(np.float64)
    chunk = max(1, 4_000_000 // (new * taps))
    refs, bounds = [], []
    for c0 in range(fa, fb, chunk):
        f = np.arange(c0, min(fb, c0 + chunk))
        idx = f[:, None] * orig - width + np.arange(taps)[None, :]
        seg = np.where((idx >= 0) & (idx < n), x64[np.clip(idx, 0, max(n - 1, 0))], 0.0)
        prod = seg[:, None, :] * k[None, :, :]                                    # [frames, new, taps]
        ps = np.cumsum(prod, axis=2)
        refs.append(ps[:, :, -1].reshape(-1))
        bounds.append(1.001 * U * (np.abs(ps).sum(2) + np.abs(prod).sum(2)).reshape(-1))
    n_out = -(-new * n // orig)
    keep = max(0, min((fb - fa) * new, n_out - fa * new))
    return np.concatenate(refs)[:keep], np.concatenate(bounds)[:keep]


def oracle_window(x, orig_sr, new_sr, fa, fb):
    """AO.resample_kaiser on the input slice that feeds output frames [fa, fb): started a whole number of frames (orig samples)
    early, at least `width` samples before frame fa's first tap, so the phases line up and no zero padding leaks in."""
    _, width, orig, new = AO.sinc_kernel(orig_sr, new_sr)
    m = min(fa, -(-width // orig))
    s0, s1 = (fa - m) * orig, min(len(x), fb * orig + width + orig)
    y = AO.resample_kaiser(x[s0:s1], orig_sr, new_sr)
    n_out = -(-new * len(x) // orig)
    keep = max(0, min((fb - fa) * new, n_out - fa * new))
    return y[m * new: m * new + keep]


def check_resample(got, q, x, orig_sr, new_sr, fa, fb, label, fixed=None):
    """got / q: the kernel's plain / PCM16 outputs for frames [fa, fb)."""
    ref, bound = resample_ref_bound(x, orig_sr, new_sr, fa, fb)
    want = oracle_window(x, orig_sr, new_sr, fa, fb)
    assert want.shape == ref.shape == got.shape, (label, want.shape, ref.shape, got.shape)
    np.testing.assert_allclose(ref, want, rtol=0, atol=1e-12)
    err = np.abs(got.astype(np.float64) - want)
    ratio = _judge(label, [("abs", err, bound)], got, want, fixed)
    if q is not None:
        lsb = np.abs(q.astype(np.float64) * 32768 - AO.pcm16_roundtrip(want) * 32768)
        t = want * 32768
        near = np.abs(t - np.floor(t) - 0.5) <= bound * 32768
        assert lsb.max() <= 1 and not ((lsb > 0) & ~near).any(), (label, float(lsb.max()), int(((lsb > 0) & ~near).sum()))
    return ratio


# ------------------------------------------------------------------------------------------------ signals
def signals(kind, n):
    """name -> float32 clip of n samples: the sparse-spectrum and boundary cases, full-scale noise, recipes.audio_clip."""
    c = FE[kind]
    sr, hop, nfft = (48000 if kind == "htsat" else 16000), c["hop"], c["nfft"]
    t = np.arange(n)
    rng = np.random.default_rng(5)
    out = {"audio_clip": R.audio_clip(901, n, sr),
           "sine_bin_centre": 0.5 * np.sin(2 * np.pi * 37 * t / nfft),
           "sine_half_bin": 0.5 * np.sin(2 * np.pi * 37.5 * t / nfft + 0.3),
           "dc_offset": np.full(n, 0.25) + 0.01 * rng.standard_normal(n),
           "nyquist": 0.5 * (1 - 2 * (t % 2)),
           "silence": np.zeros(n),
           "noise_full_scale": rng.uniform(-1, 1, n)}
    k = 37
    for name, pos in (("impulse_0", 0), ("impulse_kHOP-1", k * hop - 1), ("impulse_kHOP", k * hop), ("impulse_kHOP+1", k * hop + 1),
                      ("impulse_32HOP", 32 * hop), ("impulse_last", n - 1)):
        if pos >= n:
            continue
        z = np.zeros(n)
        z[pos] = 0.9
        out[name] = z
    return {name: v.astype(np.float32) for name, v in out.items()}


def _dev(clips):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clips]


# ------------------------------------------------------------------------------------------------ VGGish
def test_vggish_signals_and_lengths():
    from fadtk_amd import hip
    sig = signals("vggish", 15600 + 15360)                       # two examples, 192 frames: six 32-frame workgroups
    names = list(sig)
    clips = [sig[s] for s in names]
    ex, off = hip.logmel_vggish(clips)
    ex_dev, off_dev = hip.logmel_vggish(_dev(clips))
    assert np.array_equal(off_dev, off) and np.array_equal(ex_dev.cpu().numpy(), ex)
    for i, s in enumerate(names):
        check_vggish(ex[off[i]:off[i + 1]], clips[i], f"vggish {s} n={len(clips[i])}")
    lens = [0, 399, 400, 15599, 15600, 15601] + [15600 + 15360 * j + d for j in (1, 2, 5) for d in (-1, 0, 1)]
    clips = [R.audio_clip(600 + i, n, 16000) for i, n in enumerate(lens)]
    ex, off = hip.logmel_vggish(clips)
    assert [int(d) for d in np.diff(off)] == [L.vggish_num_examples(n) for n in lens]
    ex_dev, off_dev = hip.logmel_vggish(_dev(clips))
    assert np.array_equal(off_dev, off) and np.array_equal(ex_dev.cpu().numpy(), ex)
    for i, n in enumerate(lens):
        check_vggish(ex[off[i]:off[i + 1]], clips[i], f"vggish audio_clip n={n}", fixed=3e-4)


def test_vggish_batch_equals_each_clip_alone():
    """No arithmetic crosses clips: every clip's examples in a batch of 120 mixed-length clips (silence, loud noise, tones, empty
    ones) are bitwise those of the clip computed alone, on the host and the device route."""
    from fadtk_amd import hip
    rng = np.random.default_rng(77)
    lens = rng.choice([0, 399, 15599, 15600, 15601, 30960, 46321, 20000], size=120)
    clips = []
    for i, n in enumerate(lens):
        kind = i % 4
        x = R.audio_clip(700 + i, int(n), 16000) if kind == 0 else (rng.uniform(-1, 1, n) if kind == 1 else
                                                                   (np.zeros(n) if kind == 2 else 0.3 * np.sin(0.05 * i * np.arange(n))))
        clips.append(np.asarray(x, np.float32))
    ex, off = hip.logmel_vggish(clips)
    ex_dev, off_dev = hip.logmel_vggish(_dev(clips))
    assert np.array_equal(off_dev, off) and np.array_equal(ex_dev.cpu().numpy(), ex)
    for i, c in enumerate(clips):
        alone, _ = hip.logmel_vggish([c])
        assert np.array_equal(ex[off[i]:off[i + 1]], alone), i
    for i in (0, 1, 3, 5):
        check_vggish(ex[off[i]:off[i + 1]], clips[i], f"vggish batch clip {i} n={lens[i]}")


# ------------------------------------------------------------------------------------------------ Whisper
def test_whisper_signals_both_mel_counts_alternating():
    """Calls alternate between 80 and 128 mels (the per-(kind, n_mels) table cache); silence gives one value, -1.5."""
    from fadtk_amd import hip
    sig = signals("whisper", 16000 * 5 + 77)
    for s, x in sig.items():
        for n_mels in (80, 128):
            got = hip.logmel_whisper([x], n_mels=n_mels)[0]
            check_whisper(got, x, n_mels, f"whisper {s} n={len(x)} mels={n_mels}")
            if s == "silence":
                v = np.unique(got)
                assert v.size == 1 and abs(float(v[0]) + 1.5) <= 4 * 1.5 * U, v
    x = sig["audio_clip"]
    got = hip.logmel_whisper(_dev([x, sig["impulse_32HOP"]]), n_mels=128)
    assert np.array_equal(got[0].cpu().numpy(), hip.logmel_whisper([x], n_mels=128)[0])


def test_whisper_lengths_host_and_device():
    from fadtk_amd import hip
    lens = [0, 1, 479999, 480000, 480001, 960000]
    clips = [R.audio_clip(800 + i, n, 16000) for i, n in enumerate(lens)]
    for n_mels in (80, 128):
        out = hip.logmel_whisper(clips, n_mels=n_mels)
        assert out.shape == (len(lens), n_mels, 3000)
        dev = hip.logmel_whisper(_dev(clips), n_mels=n_mels)
        assert np.array_equal(dev.cpu().numpy(), out)
        for i, n in enumerate(lens):
            check_whisper(out[i], clips[i], n_mels, f"whisper audio_clip n={n} mels={n_mels}", fixed=2e-4)


def test_whisper_batch_equals_each_clip_alone():
    """The per-clip maximum stays per clip: a loud clip next to quiet ones moves no other clip's clamp."""
    from fadtk_amd import hip
    rng = np.random.default_rng(9)
    t = np.arange(160000)
    clips = [rng.uniform(-1, 1, 160000), 1e-4 * np.sin(2 * np.pi * 440 * t / 16000), np.zeros(50000),
             R.audio_clip(810, 70000, 16000), 1e-6 * rng.standard_normal(480001), np.zeros(1) + 0.5, 3e-3 * (1 - 2 * (t % 2))]
    clips = [np.asarray(c, np.float32) for c in clips]
    for n_mels in (128, 80):
        out = hip.logmel_whisper(clips, n_mels=n_mels)
        dev = hip.logmel_whisper(_dev(clips), n_mels=n_mels).cpu().numpy()
        assert np.array_equal(dev, out)
        for i, c in enumerate(clips):
            assert np.array_equal(out[i], hip.logmel_whisper([c], n_mels=n_mels)[0]), (n_mels, i)
        for i in (1, 4, 6):
            check_whisper(out[i], clips[i], n_mels, f"whisper batch quiet clip {i} mels={n_mels}")


# ------------------------------------------------------------------------------------------------ HTSAT
def test_htsat_signals_and_lengths():
    from fadtk_amd import hip
    sig = signals("htsat", 48000)
    names = list(sig)
    out = hip.logmel_htsat([sig[s] for s in names])
    dev = hip.logmel_htsat(_dev([sig[s] for s in names]))
    assert np.array_equal(dev.cpu().numpy(), out)
    for i, s in enumerate(names):
        check_htsat(out[i], sig[s], f"htsat {s} n=48000")
    for n in (513, 959, 960, 961, 1023, 1024, 1025, 480000):
        clips = [R.audio_clip(900 + n % 97, n, 48000), signals("htsat", n)["noise_full_scale"]]
        out = hip.logmel_htsat(clips)
        assert out.shape == (2, 1 + n // 480, 64)
        assert np.array_equal(hip.logmel_htsat(_dev(clips)).cpu().numpy(), out)
        check_htsat(out[0], clips[0], f"htsat audio_clip n={n}", fixed=2e-3)
        check_htsat(out[1], clips[1], f"htsat noise_full_scale n={n}")


def test_htsat_refuses_mismatched_and_short_clips():
    """A clip of 512 samples or fewer cannot be reflect-padded by 512 (torch.stft refuses it on the reference's path):
    FAD_ERR_SHAPE, raised as AssertionError; 513 is the shortest clip accepted."""
    from fadtk_amd import hip
    x = R.audio_clip(950, 2000, 48000)
    with pytest.raises(AssertionError):
        hip.logmel_htsat([x, x[:1000]])
    for n in (2, 300, 511, 512):
        with pytest.raises(AssertionError, match="512"):
            hip.logmel_htsat([x[:n]])
    check_htsat(hip.logmel_htsat([x[:513]])[0], x[:513], "htsat audio_clip n=513 (shortest accepted)")


# ------------------------------------------------------------------------------------------------ more than 32 768 clips
def test_vggish_batch_across_the_launch_split():
    """32 800 clips, mostly empty: launches split at 32 768 clips and shift offsets / frame_base / clip_frames.  Distinct
    example-sized clips on both sides of 32 767 / 32 768 against the oracle, repeats bitwise equal to their first occurrence."""
    from fadtk_amd import hip
    n = SPLIT + 32
    distinct = {0: 15600, 1: 30960, SPLIT - 2: 15601, SPLIT - 1: 30960, SPLIT: 15600, SPLIT + 1: 46320, n - 1: 15600}
    repeat = {7: 0, SPLIT - 5: 1, SPLIT + 3: SPLIT, SPLIT + 9: SPLIT - 1, n - 2: 0}
    src = {i: R.audio_clip(1000 + i % 1000, m, 16000) for i, m in distinct.items()}
    empty = np.zeros(0, np.float32)
    clips = [src.get(i, src[repeat[i]] if i in repeat else empty) for i in range(n)]
    clips[11] = np.zeros(300, np.float32)                                        # short clips: no examples
    for route, (ex, off) in (("host", hip.logmel_vggish(clips)), ("device", hip.logmel_vggish(_dev(clips)))):
        ex = ex.cpu().numpy() if route == "device" else ex
        assert int(off[-1]) == sum(L.vggish_num_examples(len(c)) for c in clips)
        for i in distinct:
            check_vggish(ex[off[i]:off[i + 1]], clips[i], f"vggish split {route} clip {i} n={len(clips[i])}")
        for i, j in repeat.items():
            assert off[i + 1] - off[i] == off[j + 1] - off[j] and np.array_equal(ex[off[i]:off[i + 1]], ex[off[j]:off[j + 1]]), (i, j)


def test_htsat_batch_across_the_launch_split():
    """32 800 clips of 513 samples built from 7 seeds, plus 4 distinct clips at 32 766 .. 32 769."""
    from fadtk_amd import hip
    n = SPLIT + 32
    base = [R.audio_clip(1100 + s, 513, 48000) for s in range(11)]
    which = [i % 7 for i in range(n)]
    for k, i in enumerate(range(SPLIT - 2, SPLIT + 2)):
        which[i] = 7 + k
    flat = np.stack([base[w] for w in which])
    for route in ("host", "device"):
        if route == "host":
            out = hip.logmel_htsat(list(flat))
        else:
            import torch
            t = torch.from_numpy(flat).cuda()
            out = hip.logmel_htsat([t[i] for i in range(n)]).cpu().numpy()
        assert out.shape == (n, 2, 64)
        first = {}
        for i, w in enumerate(which):
            if w not in first:
                first[w] = i
                check_htsat(out[i], base[w], f"htsat split {route} clip {i} (seed {w})")
            elif not np.array_equal(out[i], out[first[w]]):
                raise AssertionError(f"{route}: clip {i} differs from clip {first[w]} (same samples)")


# ------------------------------------------------------------------------------------------------ resampler
RS_PAIRS = [(16000, 44100), (22050, 48000), (11025, 48000), (44056, 16000), (96000, 16000), (48000, 16000)]
LONG = 600 * 48000 + 12345                                            # ten minutes and a bit at 48 kHz


def _rs_shape(orig_sr, new_sr):
    g = math.gcd(orig_sr, new_sr)
    orig, new = orig_sr // g, new_sr // g
    taps = AO.sinc_kernel(orig_sr, new_sr)[0].shape[1]
    fb = 8 if 7 * orig + taps <= 16384 else 1
    groups = max(1, min(256 // new if new < 256 else 1, (16384 - taps + orig) // (fb * orig)))
    return orig, new, groups * fb


@pytest.mark.parametrize("orig_sr,new_sr", RS_PAIRS)
def test_resampler_edge_pairs(orig_sr, new_sr):
    """More than 256 phases (blockIdx.y tiles), FB = 1 (44056 -> 16000: 5879 taps), many frame groups per workgroup (96 / 48 kHz
    -> 16 kHz); lengths 1, orig - 1, orig, orig + 1, a ragged last workgroup, and ten minutes at 48 kHz checked in windows."""
    import torch
    from fadtk_amd import hip
    orig, new, fpw = _rs_shape(orig_sr, new_sr)
    ragged = 3 * fpw * orig + 7 * orig // 3 + 1
    for n in sorted({1, max(1, orig - 1), orig, orig + 1, ragged}):
        x = R.audio_clip(1200 + n % 1009, n, orig_sr)
        got = hip.resample_kaiser(x, orig_sr, new_sr)
        q = hip.resample_kaiser(x, orig_sr, new_sr, quantize_pcm16=True)
        got_dev = hip.resample_kaiser(torch.from_numpy(x).cuda(), orig_sr, new_sr)
        q_dev = hip.resample_kaiser(torch.from_numpy(x).cuda(), orig_sr, new_sr, quantize_pcm16=True)
        assert np.array_equal(got_dev.cpu().numpy(), got) and np.array_equal(q_dev.cpu().numpy(), q)
        check_resample(got, q, x, orig_sr, new_sr, 0, n // orig + 1, f"resample {orig_sr}->{new_sr} n={n}")
    rng = np.random.default_rng(orig_sr + new_sr)
    x = (rng.random(LONG, dtype=np.float32) - 0.5) * np.float32(0.9)
    got = hip.resample_kaiser(x, orig_sr, new_sr)
    xd = torch.from_numpy(x).cuda()
    got_dev = hip.resample_kaiser(xd, orig_sr, new_sr).cpu().numpy()
    q_dev = hip.resample_kaiser(xd, orig_sr, new_sr, quantize_pcm16=True).cpu().numpy()
    del xd
    assert np.array_equal(got_dev, got)
    frames = LONG // orig + 1
    fw = -(-4096 // new)
    for where, fa in (("start", 0), ("middle", frames // 2 - 3), ("end", frames - fw)):
        sl = slice(fa * new, min(len(got), (fa + fw) * new))
        check_resample(got[sl], q_dev[sl], x, orig_sr, new_sr, fa, fa + fw, f"resample {orig_sr}->{new_sr} n={LONG} {where}")


@pytest.mark.parametrize("orig_sr,new_sr", [(48000, 16000), (44100, 16000), (16000, 44100)])
def test_resampler_existing_pairs_keep_the_fixed_tolerance(orig_sr, new_sr):
    """audio_clip at the lengths test_gpu_pipeline.py uses: the derived bound and the old 2e-6 both hold."""
    from fadtk_amd import hip
    n = orig_sr // 2 + 123
    x = R.audio_clip(31, n, orig_sr)
    got = hip.resample_kaiser(x, orig_sr, new_sr)
    q = hip.resample_kaiser(x, orig_sr, new_sr, quantize_pcm16=True)
    check_resample(got, q, x, orig_sr, new_sr, 0, n // _rs_shape(orig_sr, new_sr)[0] + 1,
                   f"resample {orig_sr}->{new_sr} audio_clip n={n}", fixed=2e-6 if orig_sr != 16000 else None)


@pytest.mark.parametrize("orig_sr,new_sr", [(44100, 16000), (16000, 44100), (16000, 16000)])
def test_resampler_pcm16_saturation(orig_sr, new_sr):
    """Amplitude 1.3: the PCM16 round trip clamps to -32768 and 32767 LSB, exactly as pcm16_roundtrip does."""
    from fadtk_amd import hip
    n = 3 * orig_sr // 4 + 11
    x = (1.3 * np.sin(2 * np.pi * 440 * np.arange(n) / orig_sr)).astype(np.float32)
    q = hip.resample_kaiser(x, orig_sr, new_sr, quantize_pcm16=True)
    assert q.max() == np.float32(32767 / 32768) and q.min() == np.float32(-1.0)
    if orig_sr == new_sr:
        assert np.array_equal(q, AO.pcm16_roundtrip(x).astype(np.float32))
        return
    got = hip.resample_kaiser(x, orig_sr, new_sr)
    assert np.abs(got).max() > 1.2
    check_resample(got, q, x, orig_sr, new_sr, 0, n // _rs_shape(orig_sr, new_sr)[0] + 1, f"resample {orig_sr}->{new_sr} amplitude 1.3")


# ------------------------------------------------------------------------------------------------ raw C ABI refusals
def test_raw_abi_refusals_leave_the_library_usable():
    """Each refusal returns its documented status, writes nothing, and the next call works."""
    from fadtk_amd import _capi as K
    from fadtk_amd import hip
    lib = K.load_library()
    st = K.current_stream_ptr(0)
    P64 = C.POINTER(C.c_int64)
    keep = []

    def offs(v):
        a = np.asarray(v, np.int64)
        keep.append(a)
        return a.ctypes.data_as(P64)
    probe = R.audio_clip(960, 20000, 16000)
    ref_ex, _ = hip.logmel_vggish([probe])
    wav16 = R.audio_clip(961, 20000, 16000)
    wav48 = R.audio_clip(962, 48000 + 24000, 48000)
    out = np.full(2 * 128 * 3000, 7.0, np.float32)
    cases = [
        ("whisper n_mels 64", K.FAD_ERR_INVALID, lambda: lib.fad_logmel_whisper(wav16.ctypes.data, offs([0, 20000]), 1, 64,
                                                                                  out.ctypes.data, 0, 0, st)),
        ("vggish capacity", K.FAD_ERR_SHAPE, lambda: lib.fad_logmel_vggish(wav16.ctypes.data, offs([0, 16000, 20000]), 2,
                                                                             out.ctypes.data, 0, None, 0, 0, st)),
        ("vggish decreasing offsets", K.FAD_ERR_INVALID, lambda: lib.fad_logmel_vggish(wav16.ctypes.data, offs([0, 16000, 12000]), 2,
                                                                                         out.ctypes.data, 10, None, 0, 0, st)),
        ("whisper decreasing offsets", K.FAD_ERR_INVALID, lambda: lib.fad_logmel_whisper(wav16.ctypes.data, offs([0, 9000, 8000]), 2,
                                                                                           80, out.ctypes.data, 0, 0, st)),
        ("htsat mismatched lengths", K.FAD_ERR_SHAPE, lambda: lib.fad_logmel_htsat(wav48.ctypes.data, offs([0, 48000, 72000]), 2, 101,
                                                                                     out.ctypes.data, 0, 0, st)),
        ("htsat 300 samples", K.FAD_ERR_SHAPE, lambda: lib.fad_logmel_htsat(wav48.ctypes.data, offs([0, 300]), 1, 1,
                                                                              out.ctypes.data, 0, 0, st)),
        ("htsat 512 samples", K.FAD_ERR_SHAPE, lambda: lib.fad_logmel_htsat(wav48.ctypes.data, offs([0, 512]), 1, 2,
                                                                              out.ctypes.data, 0, 0, st)),
        ("resample capacity", K.FAD_ERR_SHAPE, lambda: lib.fad_resample_kaiser(wav48.ctypes.data, 48000, 48000, 16000, 0,
                                                                                 out.ctypes.data, 15999, 0, 0, st)),
    ]
    for name, status, call in cases:
        assert call() == status, (name, K.last_error())
        assert (out == 7.0).all(), name
        ex, _ = hip.logmel_vggish([probe])
        assert np.array_equal(ex, ref_ex), name
    assert lib.fad_logmel_htsat(wav48.ctypes.data, offs([0, 300]), 1, 1, out.ctypes.data, 0, 0, st) == K.FAD_ERR_SHAPE
    assert "512" in K.last_error()


# ------------------------------------------------------------------------------------------------ concurrent callers
def test_four_threads_match_serial_results():
    """Per-thread workspaces and the locked table caches: four threads call every front end and the resampler at once, each with
    its own inputs (and its own mel count / rate pair); every result is bitwise the serial one."""
    from fadtk_amd import hip
    pairs = [(44100, 16000), (16000, 44100), (96000, 16000), (22050, 48000)]

    def work(k):
        v = [R.audio_clip(1300 + k, 15600 + 15360 * k + 7, 16000), R.audio_clip(1310 + k, 1000 * k, 16000)]
        w = [R.audio_clip(1320 + k, 100000 + 7 * k, 16000)]
        h = [R.audio_clip(1330 + k, 48000 + 480 * k, 48000)] * 2
        r = R.audio_clip(1340 + k, 50000 + k, pairs[k][0])
        ex, off = hip.logmel_vggish(v)
        return [ex, off, hip.logmel_whisper(w, n_mels=(80, 128)[k % 2]), hip.logmel_htsat(h),
                hip.resample_kaiser(r, *pairs[k]), hip.resample_kaiser(r, *pairs[k], quantize_pcm16=True)]
    serial = [work(k) for k in range(4)]
    results, errors = [[None] * 3 for _ in range(4)], []
    barrier = threading.Barrier(4)

    def run(k):
        try:
            barrier.wait()
            for it in range(3):
                results[k][it] = work(k)
        except BaseException as e:       # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=run, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(4):
        for it in range(3):
            for a, b in zip(results[k][it], serial[k]):
                assert np.array_equal(a, b), (k, it)
