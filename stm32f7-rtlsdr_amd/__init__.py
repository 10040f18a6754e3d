"""MI355X-native IQ -> FM-audio path ("sdrfm") — Python plumbing over the C-ABI in include/sdrfm.h.

The product is csrc/libsdrfm.so (hand-written HIP for gfx950 + C host shim).  This package only loads it with ctypes,
mirrors its entry points one-to-one, and adds torch plumbing (device buffers, streams, torch.distributed fan-out).
There is no CPU fallback anywhere in this package: without the built library or without a gfx950 device every compute
call raises.

The directory name contains a hyphen (it is fixed by the build contract), so import it with
``importlib.import_module("stm32f7-rtlsdr_amd")``.
"""
# (Importing this package does not touch the process environment.  A host that runs RCCL beside overlapped calls wants GPU_MAX_HW_QUEUES=8 set BEFORE the HIP
# runtime loads — INTEGRATION.md section 3 says why; bench.py and examples/multi_gpu_main.c set it themselves.)
from .lib import SdrfmError, load_library, library_path, STATUS, ABI_SYMBOLS
from .demod import FmDemod, FmConfig
from .wbfm import WbfmDemod, WbfmConfig
from .stereo import StereoDemod, StereoConfig
from .bcast import BroadcastDemod, BroadcastConfig
from .scan import ScanDemod, ScanConfig, METER_DTYPE, meter_add, meter_report, find_stations, stream_status, follow_selection, scan_grid, scan_capture, pilot_snr_db, audio_policy, hicut_policy, HIST_BINS, hist_add, hist_edges_hz, hist_report, deviation_quantile, ModulationMonitor
from .rds import RdsDemod, RdsConfig, RdsSync, RdsGroup, rds_parse, rds_encode_groups, rds_checkword, rds_group_bits
from .spectrum import SpectrumView, SpectrumConfig, power_db
from .sink import PcmSink, StereoPcmSink, pcm_deemph_s16_host, pcm_deemph_stereo_s16_host, pcm_deemph_stereo_hicut_s16_host, hicut_slew, AUDIO_METER_DTYPE, pcm_audio_meter_host, audio_meter_add, audio_meter_report, audio_alarms, AudioMonitor
from .rate import PcmRateMatcher, pcm_rate_host, step_for, ClockServo
from .taps import RTLSDR_FIR, rtlsdr_fir16, lowpass_taps, default_config, stereo_pilot_taps, stereo_diff_gain, rds_gain, rds_lowpass_taps, tuned_channel_taps, tuned_rotation, retune_carry, pilot_gain, hicut_corner_hz, rate_coef, truepeak_coef, mix_curve
from .siggen import make_iq, make_iq_stereo, make_iq_rds, make_iq_stations, impair_iq, MODES
from .frontend import ReplayFrontEnd, XferState
from .loudness import LOUDNESS_STATE_DTYPE, loudness_default_coef, pcm_loudness_host, LoudnessGate, LoudnessMonitor, loudness_alarms
from .truepeak import TRUEPEAK_DTYPE, truepeak_default_coef, truepeak_limit, pcm_truepeak_host, truepeak_add, truepeak_report, truepeak_alarms, headroom_gain_q15
from .limit import PcmLimiter, LIMIT_DTYPE, pcm_limit_host, pcm_limit_tp_host, limit_add, limit_report, limit_ceiling, limit_release, normalise_gain_q12
from .iqmeter import IqMeter, IQ_METER_DTYPE, IQ_HIST_BINS, iq_meter_host, iq_meter_add, iq_hist_add, iq_meter_report, iq_hist_report, gain_advice, nearest_gain
from .mix import PcmMixer, MIX_DTYPE, MIX_SLOT_DTYPE, pcm_mix_host, mix_add, mix_report, slew_for, fade_pairs, dead_channel_modes
from . import fanout
from . import mix
from . import rate
from . import lib

__all__ = [
    "SdrfmError", "load_library", "library_path", "STATUS", "ABI_SYMBOLS", "FmDemod", "FmConfig", "WbfmDemod", "WbfmConfig", "StereoDemod", "StereoConfig", "BroadcastDemod", "BroadcastConfig", "RdsDemod", "RdsConfig", "RdsSync", "RdsGroup", "rds_parse", "rds_encode_groups", "rds_checkword", "rds_group_bits", "rds_gain", "rds_lowpass_taps", "make_iq_rds", "SpectrumView", "SpectrumConfig", "power_db", "PcmSink", "StereoPcmSink", "pcm_deemph_s16_host", "pcm_deemph_stereo_s16_host", "RTLSDR_FIR",
    "rtlsdr_fir16", "lowpass_taps", "default_config", "stereo_pilot_taps", "stereo_diff_gain", "make_iq", "make_iq_stereo", "MODES", "ReplayFrontEnd", "XferState", "fanout",
    "tuned_channel_taps", "tuned_rotation", "make_iq_stations",
    "ScanDemod", "ScanConfig", "METER_DTYPE", "meter_add", "meter_report", "find_stations", "stream_status", "scan_grid", "scan_capture", "pilot_gain",
    "retune_carry", "follow_selection", "pilot_snr_db", "audio_policy",
    "pcm_deemph_stereo_hicut_s16_host", "hicut_slew", "hicut_corner_hz", "hicut_policy",
    "HIST_BINS", "hist_add", "hist_edges_hz", "hist_report", "deviation_quantile", "ModulationMonitor",
    "AUDIO_METER_DTYPE", "pcm_audio_meter_host", "audio_meter_add", "audio_meter_report", "audio_alarms", "AudioMonitor",
    "LOUDNESS_STATE_DTYPE", "loudness_default_coef", "pcm_loudness_host", "LoudnessGate", "LoudnessMonitor", "loudness_alarms",
    "TRUEPEAK_DTYPE", "truepeak_default_coef", "truepeak_limit", "pcm_truepeak_host", "truepeak_add", "truepeak_report", "truepeak_alarms",
    "headroom_gain_q15", "truepeak_coef",
    "PcmRateMatcher", "pcm_rate_host", "rate_coef", "step_for", "ClockServo", "rate",
    "PcmLimiter", "LIMIT_DTYPE", "pcm_limit_host", "pcm_limit_tp_host", "limit_add", "limit_report", "limit_ceiling", "limit_release", "normalise_gain_q12",
    "IqMeter", "IQ_METER_DTYPE", "IQ_HIST_BINS", "iq_meter_host", "iq_meter_add", "iq_hist_add", "iq_meter_report", "iq_hist_report", "gain_advice", "nearest_gain",
    "impair_iq",
    "PcmMixer", "MIX_DTYPE", "MIX_SLOT_DTYPE", "pcm_mix_host", "mix_add", "mix_report", "mix_curve", "slew_for", "fade_pairs", "dead_channel_modes", "mix",
]
