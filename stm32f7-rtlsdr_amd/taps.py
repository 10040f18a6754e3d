"""Tap fixtures.

RTLSDR_FIR is the only filter table the reference contains: the RTL2832's on-chip 32-tap symmetric FIR, of which the
firmware stores the first 16 coefficients (Middlewares/ST/STM32_USB_Host_Library/Class/RTLSDR/Inc/usbh_rtlsdr.h:340-345).
It is used here, divided by its sum, purely as the deterministic "16-tap" fixture of BASELINE configs 1-2.
"""
import ctypes as C
import numpy as np

from .siggen import _siggen

RTLSDR_FIR = (-54, -36, -41, -40, -32, -14, 14, 53, 101, 156, 215, 273, 327, 372, 404, 421)


def rtlsdr_fir16():
    t = np.asarray(RTLSDR_FIR, dtype=np.float64)
    return (t / t.sum()).astype(np.float32)  # sum = 2119


def lowpass_taps(n, cutoff_over_fs):
    """Hamming-windowed sinc, unity DC gain (tools/siggen/siggen.c: siggen_lowpass)."""
    out = np.zeros(int(n), dtype=np.float32)
    _siggen().siggen_lowpass(out.ctypes.data_as(C.c_void_p), C.c_uint32(int(n)), C.c_double(float(cutoff_over_fs)))
    return out


def default_config(fir_taps=64, fs=2.4e6, fir_decim=10, audio_taps=32, audio_decim=5):
    """Taps of the BASELINE configurations: T=16 -> RTLSDR_FIR/2119; otherwise a 100 kHz Hamming-sinc at fs;
    audio filter: 15 kHz Hamming-sinc at fs/fir_decim."""
    h = rtlsdr_fir16() if fir_taps == 16 else lowpass_taps(fir_taps, 100e3 / fs)
    g = lowpass_taps(audio_taps, 15e3 / (fs / fir_decim))
    return h, g


def stereo_pilot_taps(P, fs_d, f_pilot=19e3, cutoff_hz=1.5e3):
    """Complex pilot-filter taps b[k] = 2 w[k] exp(+j 2 pi f_pilot/fs_d (k - Δ)), Δ = (P-1)/2, w the unity-DC-gain Hamming low-pass
    of lowpass_taps: |q| = |b * d| is then the pilot's amplitude in radians.  Returns complex64 [P] (StereoConfig.pilot_coeffs)."""
    P = int(P)
    assert P % 2 == 1 and 1 <= P <= 255
    w = lowpass_taps(P, cutoff_hz / fs_d).astype(np.float64)
    k = np.arange(P, dtype=np.float64)
    return (2.0 * w * np.exp(1j * 2.0 * np.pi * f_pilot / fs_d * (k - (P - 1) / 2))).astype(np.complex64)


def stereo_diff_gain(D, fs, f_sub=38e3):
    """2 / H_D(f_sub): H_D(f) = sin(pi f D/fs) / (D sin(pi f/fs)) is the gain of the discriminator's D-sample boxcar (d is the phase
    step over D inputs), which leaves the L-R subcarrier weaker than L+R; this diff_gain restores the channel separation."""
    x = np.pi * f_sub / fs
    return float(2.0 / (np.sin(x * D) / (D * np.sin(x))))


def rds_gain(D, fs, f_sub=57e3):
    """2 / H_D(f_sub) at the RDS subcarrier: the same boxcar argument as stereo_diff_gain (H_D = 0.91061 -> 2.1963 at D = 10, 2.4 MS/s)."""
    return stereo_diff_gain(D, fs, f_sub)


def rds_lowpass_taps(Tr, fs_d, cutoff_hz=3.0e3):
    """The decimating low-pass behind the 57 kHz mixer: lowpass_taps at cutoff_hz / fs_d (the RDS spectrum ends at +-2.4 kHz)."""
    return lowpass_taps(Tr, cutoff_hz / fs_d)


def tuned_channel_taps(h, offset_hz, fs):
    """The channel low-pass h moved to offset_hz: hz[k] = h[k] exp(+j 2 pi offset_hz k / fs), evaluated in float64 and rounded once.
    Returns float32 [2T], (hr[k], hi[k]) pairs: one stream's row of sdrfm_bcast_tune's ctaps."""
    h = np.asarray(h, dtype=np.float32).astype(np.float64)
    k = np.arange(h.size, dtype=np.float64)
    hz = h * np.exp(1j * 2.0 * np.pi * float(offset_hz) * k / float(fs))
    out = np.empty(2 * h.size, dtype=np.float32)
    out[0::2], out[1::2] = hz.real, hz.imag
    return out


def tuned_rotation(offset_hz, fs, D):
    """The phase a tuned stream's y gains over D inputs from the offset alone, 2 pi offset_hz D / fs wrapped into [-pi, pi] in float64 and
    rounded once (sdrfm_bcast_tune's rot; the rounding never leaves the fp32 pi the library compares with)."""
    v = float(np.remainder(2.0 * np.pi * float(offset_hz) * int(D) / float(fs) + np.pi, 2.0 * np.pi) - np.pi)
    pi_f = float(np.float32(np.pi))
    return np.float32(min(max(v, -pi_f), pi_f))


def retune_carry(old_hz, new_hz, T, fs):
    """The carry of a re-tune from old_hz to new_hz (sdrfm_bcast_retune's carry): exp(+j 2 pi (new - old) (T - 1) / 2 / fs)
    in float64, rounded once — the phase by which the moved low-pass's y differs for a signal inside both passbands, for the symmetric h of
    lowpass_taps under tuned_channel_taps' convention (tap k multiplies x[n - k]).  Returns float32 [2]: (cr, ci)."""
    c = np.exp(1j * 2.0 * np.pi * (float(new_hz) - float(old_hz)) * (int(T) - 1) / 2.0 / float(fs))
    return np.array([c.real, c.imag], dtype=np.float32)


def hicut_corner_hz(alpha, hicut_q15, fs):
    """the -3 dB corner (Hz) of the stereo PCM sink's one-pole de-emphasis with a settled high-cut: the pole of
    y += a (x - y) with a = alpha hicut_q15 / 32768 lies at -ln(1 - a) fs / (2 pi); a = 1 (no memory at all) gives inf"""
    a = np.asarray(alpha, np.float64) * np.asarray(hicut_q15, np.float64) / 32768.0
    with np.errstate(divide="ignore"):
        return -np.log1p(-a) * float(fs) / (2.0 * np.pi)


def pilot_gain(D, fs, f_pilot=19e3):
    """H_D(f_pilot), the gain of the discriminator's D-sample boxcar at the pilot (the H_D of stereo_diff_gain; 0.98982 at D = 10,
    2.4 MS/s): a pilot of deviation v Hz has |q| = 2 pi v D / fs * H_D, which is how sdrfm_scan_report turns pilot_rms_rad into Hz."""
    x = np.pi * f_pilot / fs
    return float(np.sin(x * D) / (D * np.sin(x)))


def rate_coef(NT=32, LOGPH=8, cutoff=None, beta=9.0, step=1 << 32):
    """the coefficient table of the PCM rate matcher: int16 [(2^LOGPH + 1), NT] in Q15,
    coef[p][k] = Q15(h(k - NT/2 + 1 - p / 2^LOGPH)) with h(t) = cutoff sinc(cutoff t) Kaiser(beta) over |t| <= NT/2 — row p interpolates at the
    fraction p / 2^LOGPH, row 2^LOGPH is the next pair's row 0 moved by one tap.  cutoff is in units of the INPUT's Nyquist frequency; the
    default, 0.9 min(1, 2^32 / step), keeps the images of a step above one pair per output below the output's Nyquist frequency.  Each row is
    normalised to sum 1, rounded, and its largest tap adjusted so that the row sums to exactly 32768: a constant input comes out as itself."""
    NT, LOGPH = int(NT), int(LOGPH)
    if cutoff is None:
        cutoff = 0.9 * min(1.0, float(1 << 32) / float(step))
    nph = 1 << LOGPH
    t = np.arange(NT, dtype=np.float64)[None, :] - NT / 2 + 1 - np.arange(nph + 1, dtype=np.float64)[:, None] / nph
    u = np.clip(1.0 - (2.0 * t / NT) ** 2, 0.0, None)
    h = float(cutoff) * np.sinc(float(cutoff) * t) * np.i0(float(beta) * np.sqrt(u)) / np.i0(float(beta)) * (np.abs(t) <= NT / 2)
    q = np.rint(h / h.sum(axis=1, keepdims=True) * 32768.0).astype(np.int64)
    rows = np.arange(nph + 1)
    q[rows, np.argmax(q, axis=1)] += 32768 - q.sum(axis=1)
    if q.max() > 32767 or q.min() < -32768:
        raise ValueError("rate_coef: a tap does not fit Q15 (cutoff %g at %d taps)" % (cutoff, NT))
    return q.astype(np.int16)


def mix_curve(kind="equal_power"):
    """a gain curve for the PCM mix bus: uint16 [129], the knots t[j] at gain 256 j in Q15.  "equal_power" is
    round(32768 sin(pi j / 256)): two slots that crossfade pass 0.707 each at the middle, constant power for unrelated programmes.
    "linear" is 256 j, under which the curve changes nothing.  Both start at 0, end at 32768 and do not decrease, as
    sdrfm_pcm_mix_check_curve asks."""
    j = np.arange(129, dtype=np.float64)
    if kind == "equal_power":
        t = np.rint(32768.0 * np.sin(np.pi * j / 256.0))
    elif kind == "linear":
        t = 256.0 * j
    else:
        raise ValueError("mix_curve: %r is neither 'equal_power' nor 'linear'" % (kind,))
    return t.astype(np.uint16)


def truepeak_coef(n_phases=4, n_taps=12, cutoff=0.9, beta=6.0):
    """a coefficient table for the true-peak meter: int16 [n_phases, n_taps] in Q15, a windowed-sinc interpolator laid out as
    the BS.1770-4 Annex 2 table is — coef[p][k] = Q15(h(k - (n_taps - 1) / 2 + (p - (n_phases - 1) / 2) / n_phases)) with h(t) = cutoff
    sinc(cutoff t) Kaiser(beta) over |t| <= n_taps / 2, so the phases lie symmetrically about the middle of the row and row n_phases - 1 - p
    is row p reversed.  cutoff is in units of the input's Nyquist frequency.  Each row is normalised to sum 1, rounded, and its largest tap
    adjusted so that the row sums to exactly 32768: a constant input reads its own level.  ValueError where a tap does not fit Q15 or half a
    row passes the bound of sdrfm_truepeak_check_coef (sum of |coef| <= 65535)."""
    P, NT = int(n_phases), int(n_taps)
    if P not in (2, 4, 8) or NT % 4 or not 4 <= NT <= 64:
        raise ValueError("truepeak_coef: %d phases of %d taps" % (P, NT))
    t = np.arange(NT, dtype=np.float64)[None, :] - (NT - 1) / 2 + (np.arange(P, dtype=np.float64)[:, None] - (P - 1) / 2) / P
    u = np.clip(1.0 - (2.0 * t / NT) ** 2, 0.0, None)
    h = float(cutoff) * np.sinc(float(cutoff) * t) * np.i0(float(beta) * np.sqrt(u)) / np.i0(float(beta)) * (np.abs(t) <= NT / 2)
    q = np.rint(h / h.sum(axis=1, keepdims=True) * 32768.0).astype(np.int64)
    q[np.arange(P), np.argmax(q, axis=1)] += 32768 - q.sum(axis=1)
    if q.max() > 32767 or q.min() < -32768:
        raise ValueError("truepeak_coef: a tap does not fit Q15 (cutoff %g at %d taps)" % (cutoff, NT))
    if max(np.abs(q[:, :NT // 2]).sum(axis=1).max(), np.abs(q[:, NT // 2:]).sum(axis=1).max()) > 65535:
        raise ValueError("truepeak_coef: half a row passes the bound (cutoff %g at %d taps)" % (cutoff, NT))
    return q.astype(np.int16)
