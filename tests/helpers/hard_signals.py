"""The hard-signal corpus: fifteen 1.5 s utterances (16 kHz, int16) of the kinds opensmile_amd/synth.py never produces --
samples at +32767 / -32768, flat clipped tops, DC, a tone on a bin centre, +-1 LSB near-silence, single-sample clicks inside
digital zeros, exact-zero gaps inside voiced speech, F0 below the SHS range and near its top, octave jumps, a glide, a missing
fundamental. These are the inputs on which special cases decide the result (log floors, 0/0 in the spectral moments, voiced /
unvoiced run edges, noZeroSma and onlyInSegments around zeros, Viterbi transitions).

numpy only. signals() is a fixed contract: tests/golden/hard_*.npz hold what the real binary gives for exactly these samples
(tests/golden/make_golden_hard.py), and hard_pcm.npz holds the samples themselves."""
import numpy as np

FS = 16000


def _harm(f0, n, nh=10, amp=0.3, fs=FS):
    ph = 2 * np.pi * np.cumsum(np.broadcast_to(np.asarray(f0, float), (n,))) / fs
    x = sum(np.sin(h * ph) / h for h in range(1, nh + 1))
    return amp * x / np.max(np.abs(x))


def _i16(x):
    return np.rint(np.clip(x, -32768, 32767)).astype(np.int16)


def signals(n=24000, fs=FS):
    rng = np.random.default_rng(20240)
    t = np.arange(n) / fs
    s = {}
    s["clip_sine"] = _i16(4 * 32768 * np.sin(2 * np.pi * 150 * t))
    a = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    a[n // 2:] = -32768
    s["nyquist_then_min"] = a
    s["dc"] = np.full(n, 12000, np.int16)
    s["lsb_noise"] = rng.integers(-1, 2, n).astype(np.int16)
    c = np.zeros(n, np.int16)
    for k, p in enumerate(range(700, n - 400, 1733)):
        c[p] = (32767, -32768, 1, -1)[k % 4]
    s["clicks_in_zeros"] = c
    v = _harm(140.0, n) * 32767
    g = np.ones(n)
    pos = 2000
    for gap_ms in (5, 10, 20, 30, 70, 200, 1, 2):
        w = int(gap_ms * fs / 1000)
        g[pos:pos + w] = 0
        pos += w + 2400
    s["gated_voiced"] = _i16(v * g)
    s["f0_45"] = _i16(_harm(45.0, n) * 32767)
    s["f0_650"] = _i16(_harm(650.0, n, nh=6) * 32767)
    s["octave_jumps"] = _i16(_harm(np.choose((np.arange(n) // 960) % 3, [110.0, 220.0, 440.0]), n) * 32767)
    s["glide_80_600"] = _i16(_harm(80.0 * (600 / 80.0) ** (np.arange(n) / n), n) * 32767)
    ph = 2 * np.pi * 120 * t
    s["missing_fundamental"] = _i16(0.25 * 32767 * (np.sin(2 * ph) + np.sin(3 * ph) + np.sin(4 * ph)) / 3)
    s["bin_tone_lsb_then_full"] = _i16(np.concatenate([np.rint(np.sin(2 * np.pi * 1000 * t[:n // 2])),
                                                       np.rint(32767 * np.sin(2 * np.pi * 1000 * t[n // 2:]))]))
    s["slow_ramp"] = _i16(((np.arange(n) * 7) % 65536) - 32768)
    s["full_range_noise"] = rng.integers(-32768, 32768, n).astype(np.int16)
    z = np.zeros(n, np.int16)
    z[6000:18000] = _i16(_harm(200.0, 12000) * 32767)
    s["zeros_voiced_zeros"] = z
    return s


NAMES = ("clip_sine", "nyquist_then_min", "dc", "lsb_noise", "clicks_in_zeros", "gated_voiced", "f0_45", "f0_650", "octave_jumps",
         "glide_80_600", "missing_fundamental", "bin_tone_lsb_then_full", "slow_ramp", "full_range_noise", "zeros_voiced_zeros")
TAPPED = ("dc", "clicks_in_zeros", "gated_voiced", "glide_80_600", "zeros_voiced_zeros")   # ComParE level taps kept in the fixture


# ---------------------------------------------------------------- float64 restatement of the MFCC12_0_D_A tail (the fast kernel's gate)
def mfcc_tail64(power, coef, chan, cos, lif, n_bands, melfloor):
    """T x 257 power spectrum (float64) -> T x 13 cepstra [c1..c12, c0] as [melspec] + [mfcc] of MFCC12_0_D_A.conf compute
    them, everything in float64: bin m adds p * coef[m] to band chan[m] and p - p * coef[m] to band chan[m] + 1 (bins with
    chan[m] < -1 are outside the bank); the bands are scaled by 32767^2 (HTK-compatible sample scaling), floored, logged, and go
    through the DCT table, the lifter and sqrt(2 / n_bands). Also returns the mel energies before the floor."""
    power = np.asarray(power, np.float64)
    T = power.shape[0]
    mel = np.zeros((T, n_bands + 1), np.float64)
    for m in range(power.shape[1]):
        c = int(chan[m])
        if c < -1:
            continue
        a = power[:, m] * float(coef[m])
        if c >= 0:
            mel[:, c] += a
        if c + 1 < n_bands:
            mel[:, c + 1] += power[:, m] - a
    mel = mel[:, :n_bands] * (32767.0 * 32767.0)
    lm = np.log(np.maximum(mel, float(melfloor)))
    c = (lm @ np.asarray(cos, np.float64).T) * np.asarray(lif, np.float64)[None, :] * np.sqrt(2.0 / n_bands)
    return c, mel


def frame_scaled(d, ref):
    """Per-frame-scaled |d|: max_i |d[t, i]| / max_i |ref[t, i]| (tolerance.frame_scaled_err's scale), 0 where the reference frame
    is all zero; and the mask of non-zero frames."""
    s = np.abs(np.asarray(ref, np.float64)).max(axis=1)
    nz = s > 0
    e = np.zeros(len(s))
    e[nz] = np.abs(np.asarray(d, np.float64)).max(axis=1)[nz] / s[nz]
    return e, nz


def e_ref(oracle, pcm):
    """The reference's own transform rounding per frame of one utterance: the float64 tail on a float64 FFT of the oracle's
    windowed frames (`c_fft64`) against the same tail on the squares of the oracle's magnitudes (`c_mag`), per-frame-scaled by the
    oracle's static columns. Returns {e: [T], nz: non-zero-frame mask [T], c_fft64, c_mag: [T x 13], above: all mel energies above
    the floor [T], out: the oracle's output [T x 39]}."""
    cfg = oracle.default_cfg()
    out, t = oracle.mfcc_chain(cfg, pcm, taps=True)
    _, coef, chan, cos, lif = oracle.export_tables(cfg)
    floor = 1.0 if cfg.mfcc_htk_compatible else float(cfg.melfloor)       # cMfcc forces the floor to 1 in HTK mode
    spec = np.fft.rfft(t["win"].astype(np.float64), n=512, axis=1)
    c64, _ = mfcc_tail64(spec.real ** 2 + spec.imag ** 2, coef, chan, cos, lif, cfg.n_bands, floor)
    cmag, mel = mfcc_tail64(t["mag"].astype(np.float64) ** 2, coef, chan, cos, lif, cfg.n_bands, floor)
    n = cfg.last_mfcc - cfg.first_mfcc + 1
    assert cfg.first_mfcc == 0 and cfg.mfcc_htk_compatible                 # HTK order: c1 .. c12, c0
    order = list(range(1, n)) + [0]
    c64, cmag = c64[:, order], cmag[:, order]
    e, nz = frame_scaled(c64 - cmag, out[:, :n])
    return dict(e=e, nz=nz, c_fft64=c64, c_mag=cmag, above=(mel > floor).all(axis=1), out=out)
