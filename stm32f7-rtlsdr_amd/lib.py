"""ctypes binding of csrc/libsdrfm.so — one Python function per C entry point of include/sdrfm.h."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

STATUS = {
    0: "SDRFM_OK", 1: "SDRFM_BUSY", 2: "SDRFM_FAIL", 3: "SDRFM_NOT_SUPPORTED", 4: "SDRFM_UNRECOVERED_ERROR",
    16: "SDRFM_EINVAL", 17: "SDRFM_EODD", 18: "SDRFM_ECAPACITY", 19: "SDRFM_NO_DEVICE", 20: "SDRFM_ENOMEM",
}
OK, EINVAL, EODD, ECAPACITY, NO_DEVICE = 0, 16, 17, 18, 19
F_DEVICE_PTRS = 1
F_OVERLAP = 2
TUNE_SHARED_INPUT = 1   # SDRFM_TUNE_SHARED_INPUT

# every symbol include/sdrfm.h declares
ABI_SYMBOLS = [
    "sdrfm_create", "sdrfm_destroy", "sdrfm_reset", "sdrfm_audio_count", "sdrfm_process", "sdrfm_process_batch",
    "sdrfm_set_stream", "sdrfm_synchronize", "sdrfm_flush", "sdrfm_flush_previous", "sdrfm_wait_previous", "sdrfm_process_batch_pcm", "sdrfm_kernel_name", "sdrfm_abi_version", "sdrfm_strerror",
    "sdrfm_wbfm_create", "sdrfm_wbfm_destroy", "sdrfm_wbfm_reset", "sdrfm_wbfm_audio_count", "sdrfm_wbfm_process_batch",
    "sdrfm_wbfm_set_stream", "sdrfm_wbfm_synchronize", "sdrfm_wbfm_kernel_name", "sdrfm_rtl_pack_fir", "sdrfm_rtl_resampler", "sdrfm_e4k_pll_params",
    "sdrfm_shard_range",
    "sdrfm_spectrum_create", "sdrfm_spectrum_destroy", "sdrfm_spectrum_process_batch", "sdrfm_spectrum_set_stream",
    "sdrfm_spectrum_synchronize", "sdrfm_spectrum_kernel_name",
    "sdrfm_pcm_deemph_s16", "sdrfm_pcm_alpha",
    "sdrfm_pcm_sink_create", "sdrfm_pcm_sink_destroy", "sdrfm_pcm_sink_reset", "sdrfm_pcm_sink_process_batch",
    "sdrfm_pcm_sink_set_stream", "sdrfm_pcm_sink_synchronize", "sdrfm_pcm_sink_get_state",
    "sdrfm_ring_create", "sdrfm_ring_destroy", "sdrfm_ring_submit", "sdrfm_ring_collect",
    "sdrfm_stereo_create", "sdrfm_stereo_destroy", "sdrfm_stereo_reset", "sdrfm_stereo_audio_count", "sdrfm_stereo_process_batch",
    "sdrfm_stereo_set_stream", "sdrfm_stereo_synchronize", "sdrfm_stereo_kernel_name", "sdrfm_pcm_deemph_stereo_s16",
    "sdrfm_rds_create", "sdrfm_rds_destroy", "sdrfm_rds_reset", "sdrfm_rds_count", "sdrfm_rds_process_batch", "sdrfm_rds_set_stream",
    "sdrfm_rds_synchronize", "sdrfm_rds_kernel_name", "sdrfm_rds_checkword", "sdrfm_rds_syndrome", "sdrfm_rds_sync_create",
    "sdrfm_rds_sync_destroy", "sdrfm_rds_sync_reset", "sdrfm_rds_sync_push", "sdrfm_rds_sync_stats",
    "sdrfm_bcast_create", "sdrfm_bcast_destroy", "sdrfm_bcast_reset", "sdrfm_bcast_counts", "sdrfm_bcast_process_batch",
    "sdrfm_bcast_set_stream", "sdrfm_bcast_synchronize", "sdrfm_bcast_kernel_name", "sdrfm_bcast_tune",
    "sdrfm_pcm_stereo_sink_create", "sdrfm_pcm_stereo_sink_destroy", "sdrfm_pcm_stereo_sink_reset", "sdrfm_pcm_stereo_sink_process_batch",
    "sdrfm_pcm_stereo_sink_set_stream", "sdrfm_pcm_stereo_sink_synchronize", "sdrfm_pcm_stereo_sink_get_state",
    "sdrfm_stereo_process_batch_pcm", "sdrfm_bcast_process_batch_pcm",
    "sdrfm_scan_create", "sdrfm_scan_destroy", "sdrfm_scan_reset", "sdrfm_scan_tune", "sdrfm_scan_process_batch", "sdrfm_scan_set_stream",
    "sdrfm_scan_synchronize", "sdrfm_scan_kernel_name", "sdrfm_scan_report", "sdrfm_scan_meter_add",
    "sdrfm_bcast_process_batch_metered", "sdrfm_bcast_retune", "sdrfm_bcast_set_audio", "sdrfm_bcast_get_audio",
    "sdrfm_pcm_deemph_stereo_hicut_s16", "sdrfm_pcm_stereo_sink_set_hicut", "sdrfm_pcm_stereo_sink_get_hicut",
    "sdrfm_scan_process_batch_hist", "sdrfm_scan_hist_add", "sdrfm_scan_hist_report",
    "sdrfm_bcast_process_batch_metered_hist", "sdrfm_bcast_hist_kernel_name",
    "sdrfm_pcm_audio_meter_s16", "sdrfm_audio_meter_add", "sdrfm_audio_meter_report",
    "sdrfm_pcm_stereo_sink_meter_enable", "sdrfm_pcm_stereo_sink_meter_disable", "sdrfm_pcm_stereo_sink_meter_read",
    "sdrfm_loudness_default_coef", "sdrfm_loudness_check_coef", "sdrfm_loudness_check_domain", "sdrfm_pcm_loudness_s16", "sdrfm_loudness_gate_create", "sdrfm_loudness_gate_push",
    "sdrfm_loudness_gate_report", "sdrfm_loudness_gate_reset", "sdrfm_loudness_gate_free", "sdrfm_pcm_stereo_sink_loudness_enable",
    "sdrfm_pcm_stereo_sink_loudness_disable", "sdrfm_pcm_stereo_sink_loudness_read", "sdrfm_pcm_stereo_sink_loudness_get_state",
    "sdrfm_truepeak_default_coef", "sdrfm_truepeak_check_coef", "sdrfm_truepeak_limit", "sdrfm_pcm_truepeak_s16", "sdrfm_truepeak_add",
    "sdrfm_truepeak_report", "sdrfm_pcm_stereo_sink_truepeak_enable", "sdrfm_pcm_stereo_sink_truepeak_disable",
    "sdrfm_pcm_stereo_sink_truepeak_read",
    "sdrfm_pcm_rate_create", "sdrfm_pcm_rate_destroy", "sdrfm_pcm_rate_reset", "sdrfm_pcm_rate_set_step", "sdrfm_pcm_rate_count",
    "sdrfm_pcm_rate_process_batch", "sdrfm_pcm_rate_get_state", "sdrfm_pcm_rate_set_stream", "sdrfm_pcm_rate_synchronize",
    "sdrfm_pcm_rate_kernel_name", "sdrfm_pcm_rate_s16", "sdrfm_pcm_rate_check_coef",
    "sdrfm_pcm_limit_create", "sdrfm_pcm_limit_destroy", "sdrfm_pcm_limit_reset", "sdrfm_pcm_limit_set_params", "sdrfm_pcm_limit_set_gain",
    "sdrfm_pcm_limit_get_params", "sdrfm_pcm_limit_process_batch", "sdrfm_pcm_limit_read", "sdrfm_pcm_limit_get_state",
    "sdrfm_pcm_limit_set_stream", "sdrfm_pcm_limit_synchronize", "sdrfm_pcm_limit_kernel_name", "sdrfm_pcm_limit_s16",
    "sdrfm_pcm_limit_state_words", "sdrfm_pcm_limit_state_init", "sdrfm_pcm_limit_check_params", "sdrfm_pcm_limit_add",
    "sdrfm_pcm_limit_report", "sdrfm_pcm_limit_ceiling",
    "sdrfm_pcm_tplimit_create", "sdrfm_pcm_tplimit_get_detector", "sdrfm_pcm_tplimit_s16", "sdrfm_pcm_tplimit_state_words",
    "sdrfm_pcm_tplimit_state_init", "sdrfm_pcm_tplimit_latency",
    "sdrfm_iq_meter_create", "sdrfm_iq_meter_destroy", "sdrfm_iq_meter_process_batch", "sdrfm_iq_meter_set_stream", "sdrfm_iq_meter_synchronize",
    "sdrfm_iq_meter_kernel_name", "sdrfm_iq_meter_u8", "sdrfm_iq_meter_add", "sdrfm_iq_hist_add", "sdrfm_iq_meter_report", "sdrfm_iq_hist_report",
    "sdrfm_pcm_mix_create", "sdrfm_pcm_mix_destroy", "sdrfm_pcm_mix_reset", "sdrfm_pcm_mix_set_routes", "sdrfm_pcm_mix_set_gains",
    "sdrfm_pcm_mix_get_slots", "sdrfm_pcm_mix_process_batch", "sdrfm_pcm_mix_read", "sdrfm_pcm_mix_set_stream", "sdrfm_pcm_mix_synchronize",
    "sdrfm_pcm_mix_kernel_name", "sdrfm_pcm_mix_s16", "sdrfm_pcm_mix_check_slots", "sdrfm_pcm_mix_check_curve", "sdrfm_pcm_mix_add",
    "sdrfm_pcm_mix_report",
]


# include/sdrfm_dev.h: test hooks the product library also exports / development-library-only aids (not the drop-in boundary)
TEST_HOOK_SYMBOLS = ["sdrfm_host_atan2f", "sdrfm_host_discriminate", "sdrfm_debug_discriminate", "sdrfm_q_build", "sdrfm_q_seed", "sdrfm_q_guard", "sdrfm_q_guard2", "sdrfm_debug_q_guard", "sdrfm_debug_read_ceiling", "sdrfm_debug_route", "sdrfm_sink_chain_tables"]
DEV_ONLY_SYMBOLS = ["sdrfm_debug_phase_cycles", "sdrfm_debug_raw", "sdrfm_dev_read_debug"]


class SdrfmError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = int(status)
        name = STATUS.get(self.status, "status %d" % self.status)
        msg = ""
        try:
            msg = load_library().sdrfm_strerror(self.status).decode()
        except Exception:  # pragma: no cover
            pass
        super().__init__("%s%s (%s)" % (where + ": " if where else "", name, msg))


class Handle:
    """The lifecycle the handle classes share: the C handle in _h, destroyed once by close, on deletion or at the end of a with block; _ck turns a
    status into an SdrfmError.  A class names its C destroy function in _destroy, as a literal."""
    _destroy = None

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, st, where):
        if st != OK:
            raise SdrfmError(st, where)


class StreamHandle(Handle):
    """A Handle whose C handle has <prefix>_set_stream and <prefix>_synchronize; the class names the prefix in _prefix, as a literal."""
    _prefix = None

    def set_stream(self, ptr):
        where = self._prefix + "_set_stream"
        self._ck(getattr(self._lib, where)(self._h, C.c_void_p(int(ptr) if ptr else None)), where)

    def synchronize(self):
        where = self._prefix + "_synchronize"
        self._ck(getattr(self._lib, where)(self._h), where)


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_streams", C.c_uint32), ("fir_taps", C.c_uint32), ("fir_decim", C.c_uint32),
        ("fir_coeffs", C.POINTER(C.c_float)), ("audio_taps", C.c_uint32), ("audio_decim", C.c_uint32),
        ("audio_coeffs", C.POINTER(C.c_float)), ("max_bytes_per_call", C.c_uint32), ("device", C.c_int32),
        ("flags", C.c_uint32),
    ]


class WbfmConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_streams", C.c_uint32), ("proto_taps", C.c_uint32),
        ("proto_coeffs", C.POINTER(C.c_float)), ("resamp_taps", C.c_uint32), ("resamp_up", C.c_uint32),
        ("resamp_down", C.c_uint32), ("resamp_coeffs", C.POINTER(C.c_float)), ("max_bytes_per_call", C.c_uint32),
        ("device", C.c_int32), ("flags", C.c_uint32),
    ]


class SpectrumConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_streams", C.c_uint32), ("nfft", C.c_uint32), ("window", C.POINTER(C.c_float)),
        ("max_bytes_per_call", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32),
    ]


class StereoConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_streams", C.c_uint32), ("fir_taps", C.c_uint32), ("fir_decim", C.c_uint32),
        ("fir_coeffs", C.POINTER(C.c_float)), ("pilot_taps", C.c_uint32), ("pilot_coeffs", C.POINTER(C.c_float)),
        ("pilot_min", C.c_float), ("diff_gain", C.c_float), ("audio_taps", C.c_uint32), ("audio_decim", C.c_uint32),
        ("audio_coeffs", C.POINTER(C.c_float)), ("max_bytes_per_call", C.c_uint32), ("device", C.c_int32),
        ("flags", C.c_uint32),
    ]


class RdsConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_streams", C.c_uint32), ("fir_taps", C.c_uint32), ("fir_decim", C.c_uint32),
        ("fir_coeffs", C.POINTER(C.c_float)), ("pilot_taps", C.c_uint32), ("pilot_coeffs", C.POINTER(C.c_float)),
        ("pilot_min", C.c_float), ("rds_gain", C.c_float), ("rds_taps", C.c_uint32), ("rds_decim", C.c_uint32),
        ("rds_coeffs", C.POINTER(C.c_float)), ("max_bytes_per_call", C.c_uint32), ("device", C.c_int32),
        ("flags", C.c_uint32),
    ]


class BcastConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_streams", C.c_uint32), ("fir_taps", C.c_uint32), ("fir_decim", C.c_uint32),
        ("fir_coeffs", C.POINTER(C.c_float)), ("pilot_taps", C.c_uint32), ("pilot_coeffs", C.POINTER(C.c_float)),
        ("pilot_min", C.c_float), ("diff_gain", C.c_float), ("audio_taps", C.c_uint32), ("audio_decim", C.c_uint32),
        ("audio_coeffs", C.POINTER(C.c_float)), ("rds_gain", C.c_float), ("rds_taps", C.c_uint32), ("rds_decim", C.c_uint32),
        ("rds_coeffs", C.POINTER(C.c_float)), ("max_bytes_per_call", C.c_uint32), ("device", C.c_int32),
        ("flags", C.c_uint32),
    ]


class ScanConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_streams", C.c_uint32), ("fir_taps", C.c_uint32), ("fir_decim", C.c_uint32),
        ("ctaps", C.POINTER(C.c_float)), ("rot", C.POINTER(C.c_float)), ("pilot_taps", C.c_uint32), ("pilot_coeffs", C.POINTER(C.c_float)),
        ("pilot_min", C.c_float), ("max_bytes_per_call", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32),
    ]


class ScanMeter(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_pilot", C.c_uint64), ("rf_q", C.c_int64), ("freq_q", C.c_int64), ("dev_q", C.c_int64),
                ("pilot_q", C.c_int64), ("pilot2_q", C.c_int64), ("reserved", C.c_uint64)]


class ScanReport(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("level_dbfs", "freq_err_hz", "dev_rms_hz", "pilot_rms_rad", "pilot_dev_hz", "pilot_frac",
                                          "pilot_steadiness")]


class ScanHistReport(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(n, C.c_double) for n in ("centre_hz", "peak_pos_hz", "peak_neg_hz", "peak_hz", "over_min", "over_max",
                                                                  "mpx_power_dbr")]


class AudioRuns(C.Structure):
    _fields_ = [("count", C.c_uint64), ("lead", C.c_uint64), ("trail", C.c_uint64), ("longest", C.c_uint64)]


class AudioMeter(C.Structure):
    _fields_ = [("n", C.c_uint64), ("sum_l", C.c_int64), ("sum_r", C.c_int64), ("sq_l", C.c_uint64), ("sq_r", C.c_uint64), ("cross", C.c_int64),
                ("peak_l", C.c_uint32), ("peak_r", C.c_uint32), ("clip_l", C.c_uint64), ("clip_r", C.c_uint64),
                ("quiet_l", AudioRuns), ("quiet_r", AudioRuns), ("quiet_both", AudioRuns), ("reserved", C.c_uint64 * 3)]


# sdrfm_audio_meter as a structured dtype: StereoPcmSink.read_meters returns an array of these
AUDIO_RUNS_DTYPE = np.dtype([("count", "<u8"), ("lead", "<u8"), ("trail", "<u8"), ("longest", "<u8")])
AUDIO_METER_DTYPE = np.dtype([("n", "<u8"), ("sum_l", "<i8"), ("sum_r", "<i8"), ("sq_l", "<u8"), ("sq_r", "<u8"), ("cross", "<i8"),
                              ("peak_l", "<u4"), ("peak_r", "<u4"), ("clip_l", "<u8"), ("clip_r", "<u8"), ("quiet_l", AUDIO_RUNS_DTYPE),
                              ("quiet_r", AUDIO_RUNS_DTYPE), ("quiet_both", AUDIO_RUNS_DTYPE), ("reserved", "<u8", (3,))])
assert AUDIO_METER_DTYPE.itemsize == C.sizeof(AudioMeter) == 192
AMETER_F_RESET = 8      # SDRFM_AMETER_F_RESET


class AudioReport(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("rms_l_dbfs", "rms_r_dbfs", "peak_l_dbfs", "peak_r_dbfs", "dc_l", "dc_r", "rail_l", "rail_r",
                                          "quiet_l", "quiet_r", "quiet_both", "longest_l_s", "longest_r_s", "longest_both_s",
                                          "trail_l_s", "trail_r_s", "trail_both_s", "correlation", "mid_dbfs", "side_dbfs", "side_mid_db")]


class LoudnessCoef(C.Structure):
    _fields_ = [("c", C.c_double * 10)]


class LoudnessState(C.Structure):
    _fields_ = [("pos", C.c_uint64), ("z", (C.c_double * 4) * 2), ("e", C.c_double * 2)]


class LoudnessBlock(C.Structure):
    _fields_ = [("e_l", C.c_double), ("e_r", C.c_double)]


class LoudnessReport(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("m", "s", "i", "lra", "max_m", "max_s")] + [
        (n, C.c_uint64) for n in ("n_blocks", "n_gating", "n_abs", "n_rel", "n_short", "n_short_abs", "n_short_rel")]


# sdrfm_loudness_state and sdrfm_loudness_block as structured dtypes
LOUDNESS_STATE_DTYPE = np.dtype([("pos", "<u8"), ("z", "<f8", (2, 4)), ("e", "<f8", (2,))])
LOUDNESS_BLOCK_DTYPE = np.dtype([("e_l", "<f8"), ("e_r", "<f8")])
assert LOUDNESS_STATE_DTYPE.itemsize == C.sizeof(LoudnessState) == 88 and LOUDNESS_BLOCK_DTYPE.itemsize == C.sizeof(LoudnessBlock) == 16


class TruePeak(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n", "peak_l", "peak_r", "at_l", "at_r", "over_l", "over_r", "reserved")]


class TruePeakReport(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("dbtp_l", "dbtp_r", "dbtp", "over_frac_l", "over_frac_r", "at_seconds_l", "at_seconds_r")]


# sdrfm_truepeak as a structured dtype
TRUEPEAK_DTYPE = np.dtype([(n, "<u8") for n, _ in TruePeak._fields_])
assert TRUEPEAK_DTYPE.itemsize == C.sizeof(TruePeak) == 64


class PcmRateConfig(C.Structure):
    _fields_ = [("n_streams", C.c_uint32), ("n_taps", C.c_uint32), ("log2_phases", C.c_uint32), ("flags", C.c_uint32),
                ("coef", C.POINTER(C.c_int16)), ("device", C.c_int32)]


class PcmLimitConfig(C.Structure):
    _fields_ = [("n_streams", C.c_uint32), ("log2_window", C.c_uint32), ("gain_slew", C.c_uint32), ("flags", C.c_uint32), ("device", C.c_int32)]


class PcmLimitParams(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("ceiling", "release", "gain0", "gain_t")]


class PcmLimitRec(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n", "limited", "min_gain", "at")]


class PcmLimitReport(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("reduction_db", "limited_frac", "at_seconds")]


# sdrfm_pcm_limit_rec and sdrfm_pcm_limit_params as structured dtypes
LIMIT_DTYPE = np.dtype([(n, "<u8") for n, _ in PcmLimitRec._fields_])
LIMIT_PARAMS_DTYPE = np.dtype([(n, "<u4") for n, _ in PcmLimitParams._fields_])
assert LIMIT_DTYPE.itemsize == C.sizeof(PcmLimitRec) == 32 and LIMIT_PARAMS_DTYPE.itemsize == C.sizeof(PcmLimitParams) == 16


class IqMeterConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_streams", C.c_uint32), ("max_bytes_per_call", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32)]


class IqMeter(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n", "sum_i", "sum_q", "sum_ii", "sum_qq", "sum_iq", "rail_i", "rail_q")]


class IqReport(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("dc_i", "dc_q", "rms_dbfs", "total_dbfs", "rail_share_i", "rail_share_q", "gain_db", "skew_rad",
                                          "image_rejection_db")]


class IqHistReport(C.Structure):
    _fields_ = [("n", C.c_uint64)] + [(n, C.c_double) for n in ("peak_i", "peak_q", "level999_i", "level999_q", "codes_i", "codes_q",
                                                                  "headroom_db_i", "headroom_db_q")]


# sdrfm_iq_meter as a structured dtype
IQ_METER_DTYPE = np.dtype([(n, "<u8") for n, _ in IqMeter._fields_])
assert IQ_METER_DTYPE.itemsize == C.sizeof(IqMeter) == 64
IQ_HIST_BINS = 512      # SDRFM_IQ_HIST_BINS


class PcmMixConfig(C.Structure):
    _fields_ = [("n_in", C.c_uint32), ("n_bus", C.c_uint32), ("n_slots", C.c_uint32), ("slew", C.c_uint32), ("flags", C.c_uint32), ("device", C.c_int32)]


class PcmMixSlot(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("src", "mode", "g0", "gt")]


class PcmMixRec(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n", "clipped_l", "clipped_r", "peak")]


class PcmMixReport(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("peak_dbfs", "clipped_frac")]


# sdrfm_pcm_mix_rec and sdrfm_pcm_mix_slot as structured dtypes
MIX_DTYPE = np.dtype([(n, "<u8") for n, _ in PcmMixRec._fields_])
MIX_SLOT_DTYPE = np.dtype([(n, "<u4") for n, _ in PcmMixSlot._fields_])
assert MIX_DTYPE.itemsize == C.sizeof(PcmMixRec) == 32 and MIX_SLOT_DTYPE.itemsize == C.sizeof(PcmMixSlot) == 16
MIX_SPAN = 2048               # SDRFM_PCM_MIX_SPAN
MIX_NONE = 0xFFFFFFFF         # SDRFM_PCM_MIX_NONE
MIX_CURVE_LEN = 129           # SDRFM_PCM_MIX_CURVE_LEN


class RdsGroup(C.Structure):
    _fields_ = [("block", C.c_uint16 * 4), ("ok_mask", C.c_uint8), ("version_b", C.c_uint8)]


class RdsSyncInfo(C.Structure):
    _fields_ = [("bits", C.c_uint64), ("blocks_ok", C.c_uint64), ("blocks_failed", C.c_uint64), ("in_sync", C.c_uint32),
                ("groups", C.c_uint32)]


def library_path(dev=False):
    """csrc/libsdrfm.so (the product) or, with dev=True, csrc/libsdrfm_dev.so (same sources built with -DSDRFM_DEV: adds the
    instrumented / ablation kernels and the SDRFM_* environment knobs that the scripts under tools/ use)."""
    return os.path.join(_HERE, "csrc", "libsdrfm_dev.so" if dev else "libsdrfm.so")


_libs = {}


def load_library(dev=False):
    """Load libsdrfm.so (or the development build) or raise — never substitute anything else for it."""
    if dev in _libs:
        return _libs[dev]
    path = library_path(dev)
    if not os.path.exists(path):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C stm32f7-rtlsdr_amd/csrc%s`). There is no fallback implementation." % (path, " dev" if dev else ""))
    lib = C.CDLL(path)
    vp, u32, u32p = C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)
    lib.sdrfm_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.sdrfm_create.restype = C.c_int
    lib.sdrfm_destroy.argtypes = [vp]
    lib.sdrfm_destroy.restype = None
    lib.sdrfm_reset.argtypes = [vp]
    lib.sdrfm_reset.restype = C.c_int
    lib.sdrfm_audio_count.argtypes = [vp, u32, u32p]
    lib.sdrfm_audio_count.restype = C.c_int
    lib.sdrfm_process.argtypes = [vp, vp, u32, vp, u32, u32p]
    lib.sdrfm_process.restype = C.c_int
    lib.sdrfm_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, C.c_size_t, u32p, u32]
    lib.sdrfm_process_batch.restype = C.c_int
    lib.sdrfm_set_stream.argtypes = [vp, vp]
    lib.sdrfm_set_stream.restype = C.c_int
    lib.sdrfm_synchronize.argtypes = [vp]
    lib.sdrfm_synchronize.restype = C.c_int
    lib.sdrfm_flush.argtypes = [vp]
    lib.sdrfm_flush.restype = C.c_int
    lib.sdrfm_flush_previous.argtypes = [vp]
    lib.sdrfm_flush_previous.restype = C.c_int
    lib.sdrfm_wait_previous.argtypes = [vp, vp]
    lib.sdrfm_wait_previous.restype = C.c_int
    lib.sdrfm_process_batch_pcm.argtypes = [vp, vp, vp, C.c_size_t, C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_uint32), C.c_uint32]
    lib.sdrfm_process_batch_pcm.restype = C.c_int
    lib.sdrfm_kernel_name.argtypes = [vp]
    lib.sdrfm_kernel_name.restype = C.c_char_p
    lib.sdrfm_abi_version.argtypes = []
    lib.sdrfm_abi_version.restype = u32
    lib.sdrfm_strerror.argtypes = [C.c_int]
    lib.sdrfm_strerror.restype = C.c_char_p
    lib.sdrfm_host_atan2f.argtypes = [C.c_float, C.c_float]
    lib.sdrfm_host_atan2f.restype = C.c_float
    lib.sdrfm_host_discriminate.argtypes = [C.c_float] * 4
    lib.sdrfm_host_discriminate.restype = C.c_float
    lib.sdrfm_sink_chain_tables.argtypes = [C.c_float] + [C.POINTER(C.c_float)] * 3
    lib.sdrfm_sink_chain_tables.restype = C.c_int
    if dev:
        lib.sdrfm_debug_phase_cycles.argtypes = [vp, C.POINTER(C.c_uint64)]
        lib.sdrfm_debug_phase_cycles.restype = C.c_int
        lib.sdrfm_debug_raw.argtypes = [vp, C.POINTER(C.c_uint64)]
        lib.sdrfm_debug_raw.restype = C.c_int
    lib.sdrfm_q_build.argtypes = [vp, u32, u32, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), u32p]
    lib.sdrfm_q_build.restype = C.c_int
    lib.sdrfm_q_seed.argtypes = [vp, u32, u32, C.POINTER(C.c_int32)]
    lib.sdrfm_q_seed.restype = C.c_int
    lib.sdrfm_debug_discriminate.argtypes = [C.c_int] + [vp] * 6 + [u32]
    lib.sdrfm_debug_discriminate.restype = C.c_int
    lib.sdrfm_q_guard.argtypes = [vp, u32, vp, u32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.sdrfm_q_guard.restype = C.c_int
    lib.sdrfm_q_guard2.argtypes = [vp, u32, vp, u32, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.sdrfm_q_guard2.restype = C.c_int
    lib.sdrfm_debug_read_ceiling.argtypes = [C.c_int, C.POINTER(vp), u32, C.c_size_t, u32, C.POINTER(C.c_double)]
    lib.sdrfm_debug_read_ceiling.restype = C.c_int
    lib.sdrfm_debug_q_guard.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.sdrfm_debug_q_guard.restype = C.c_int
    lib.sdrfm_debug_route.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
    lib.sdrfm_debug_route.restype = C.c_int
    lib.sdrfm_wbfm_create.argtypes = [C.POINTER(WbfmConfig), C.POINTER(vp)]
    lib.sdrfm_wbfm_create.restype = C.c_int
    lib.sdrfm_wbfm_destroy.argtypes = [vp]
    lib.sdrfm_wbfm_destroy.restype = None
    lib.sdrfm_wbfm_reset.argtypes = [vp]
    lib.sdrfm_wbfm_reset.restype = C.c_int
    lib.sdrfm_wbfm_audio_count.argtypes = [vp, u32, u32p]
    lib.sdrfm_wbfm_audio_count.restype = C.c_int
    lib.sdrfm_wbfm_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, C.c_size_t, u32p, u32]
    lib.sdrfm_wbfm_process_batch.restype = C.c_int
    lib.sdrfm_wbfm_set_stream.argtypes = [vp, vp]
    lib.sdrfm_wbfm_set_stream.restype = C.c_int
    lib.sdrfm_wbfm_synchronize.argtypes = [vp]
    lib.sdrfm_wbfm_synchronize.restype = C.c_int
    lib.sdrfm_wbfm_kernel_name.argtypes = [vp]
    lib.sdrfm_wbfm_kernel_name.restype = C.c_char_p
    lib.sdrfm_spectrum_create.argtypes = [C.POINTER(SpectrumConfig), C.POINTER(vp)]
    lib.sdrfm_spectrum_create.restype = C.c_int
    lib.sdrfm_spectrum_destroy.argtypes = [vp]
    lib.sdrfm_spectrum_destroy.restype = None
    lib.sdrfm_spectrum_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, C.c_size_t, u32p, u32]
    lib.sdrfm_spectrum_process_batch.restype = C.c_int
    lib.sdrfm_spectrum_set_stream.argtypes = [vp, vp]
    lib.sdrfm_spectrum_set_stream.restype = C.c_int
    lib.sdrfm_spectrum_synchronize.argtypes = [vp]
    lib.sdrfm_spectrum_synchronize.restype = C.c_int
    lib.sdrfm_spectrum_kernel_name.argtypes = [vp]
    lib.sdrfm_spectrum_kernel_name.restype = C.c_char_p
    lib.sdrfm_rtl_pack_fir.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_uint8)]
    lib.sdrfm_rtl_pack_fir.restype = C.c_int
    lib.sdrfm_rtl_resampler.argtypes = [u32, u32, u32p, u32p, C.POINTER(C.c_double)]
    lib.sdrfm_rtl_resampler.restype = C.c_int
    lib.sdrfm_e4k_pll_params.argtypes = [u32, u32, vp]
    lib.sdrfm_e4k_pll_params.restype = C.c_int
    lib.sdrfm_shard_range.argtypes = [u32, u32, u32, u32p, u32p]
    lib.sdrfm_shard_range.restype = C.c_int
    lib.sdrfm_pcm_deemph_s16.argtypes = [vp, u32, C.c_float, C.c_float, C.POINTER(C.c_float), vp]
    lib.sdrfm_pcm_deemph_s16.restype = C.c_int
    lib.sdrfm_pcm_deemph_stereo_s16.argtypes = [vp, vp, u32, C.c_float, C.c_float, C.POINTER(C.c_float), vp]
    lib.sdrfm_pcm_deemph_stereo_s16.restype = C.c_int
    lib.sdrfm_stereo_create.argtypes = [C.POINTER(StereoConfig), C.POINTER(vp)]
    lib.sdrfm_stereo_create.restype = C.c_int
    lib.sdrfm_stereo_destroy.argtypes = [vp]
    lib.sdrfm_stereo_destroy.restype = None
    lib.sdrfm_stereo_reset.argtypes = [vp]
    lib.sdrfm_stereo_reset.restype = C.c_int
    lib.sdrfm_stereo_audio_count.argtypes = [vp, u32, u32p]
    lib.sdrfm_stereo_audio_count.restype = C.c_int
    lib.sdrfm_stereo_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, vp, C.c_size_t, vp, u32p, u32]
    lib.sdrfm_stereo_process_batch.restype = C.c_int
    lib.sdrfm_stereo_set_stream.argtypes = [vp, vp]
    lib.sdrfm_stereo_set_stream.restype = C.c_int
    lib.sdrfm_stereo_synchronize.argtypes = [vp]
    lib.sdrfm_stereo_synchronize.restype = C.c_int
    lib.sdrfm_stereo_kernel_name.argtypes = [vp]
    lib.sdrfm_stereo_kernel_name.restype = C.c_char_p
    lib.sdrfm_rds_create.argtypes = [C.POINTER(RdsConfig), C.POINTER(vp)]
    lib.sdrfm_rds_create.restype = C.c_int
    lib.sdrfm_rds_destroy.argtypes = [vp]
    lib.sdrfm_rds_destroy.restype = None
    lib.sdrfm_rds_reset.argtypes = [vp]
    lib.sdrfm_rds_reset.restype = C.c_int
    lib.sdrfm_rds_count.argtypes = [vp, u32, u32p]
    lib.sdrfm_rds_count.restype = C.c_int
    lib.sdrfm_rds_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, C.c_size_t, vp, u32p, u32]
    lib.sdrfm_rds_process_batch.restype = C.c_int
    lib.sdrfm_rds_set_stream.argtypes = [vp, vp]
    lib.sdrfm_rds_set_stream.restype = C.c_int
    lib.sdrfm_rds_synchronize.argtypes = [vp]
    lib.sdrfm_rds_synchronize.restype = C.c_int
    lib.sdrfm_rds_kernel_name.argtypes = [vp]
    lib.sdrfm_rds_kernel_name.restype = C.c_char_p
    lib.sdrfm_bcast_create.argtypes = [C.POINTER(BcastConfig), C.POINTER(vp)]
    lib.sdrfm_bcast_create.restype = C.c_int
    lib.sdrfm_bcast_destroy.argtypes = [vp]
    lib.sdrfm_bcast_destroy.restype = None
    lib.sdrfm_bcast_reset.argtypes = [vp]
    lib.sdrfm_bcast_reset.restype = C.c_int
    lib.sdrfm_bcast_counts.argtypes = [vp, u32, u32p, u32p]
    lib.sdrfm_bcast_counts.restype = C.c_int
    lib.sdrfm_bcast_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, vp, C.c_size_t, vp, C.c_size_t, vp, u32p, u32p, u32]
    lib.sdrfm_bcast_process_batch.restype = C.c_int
    lib.sdrfm_bcast_set_stream.argtypes = [vp, vp]
    lib.sdrfm_bcast_set_stream.restype = C.c_int
    lib.sdrfm_bcast_synchronize.argtypes = [vp]
    lib.sdrfm_bcast_synchronize.restype = C.c_int
    lib.sdrfm_bcast_kernel_name.argtypes = [vp]
    lib.sdrfm_bcast_kernel_name.restype = C.c_char_p
    lib.sdrfm_bcast_tune.argtypes = [vp, vp, vp, u32]
    lib.sdrfm_bcast_tune.restype = C.c_int
    lib.sdrfm_rds_checkword.argtypes = [C.c_uint16, C.c_int]
    lib.sdrfm_rds_checkword.restype = C.c_uint16
    lib.sdrfm_rds_syndrome.argtypes = [u32]
    lib.sdrfm_rds_syndrome.restype = C.c_uint16
    lib.sdrfm_rds_sync_create.argtypes = [C.c_double, C.POINTER(vp)]
    lib.sdrfm_rds_sync_create.restype = C.c_int
    lib.sdrfm_rds_sync_destroy.argtypes = [vp]
    lib.sdrfm_rds_sync_destroy.restype = None
    lib.sdrfm_rds_sync_reset.argtypes = [vp]
    lib.sdrfm_rds_sync_reset.restype = C.c_int
    lib.sdrfm_rds_sync_push.argtypes = [vp, vp, u32, C.POINTER(RdsGroup), u32, u32p]
    lib.sdrfm_rds_sync_push.restype = C.c_int
    lib.sdrfm_rds_sync_stats.argtypes = [vp, C.POINTER(RdsSyncInfo)]
    lib.sdrfm_rds_sync_stats.restype = C.c_int
    lib.sdrfm_pcm_alpha.argtypes = [C.c_float, C.c_float]
    lib.sdrfm_pcm_alpha.restype = C.c_float
    lib.sdrfm_ring_create.argtypes = [vp, u32, u32, C.POINTER(vp)]
    lib.sdrfm_ring_create.restype = C.c_int
    lib.sdrfm_ring_destroy.argtypes = [vp]
    lib.sdrfm_ring_destroy.restype = None
    lib.sdrfm_ring_submit.argtypes = [vp, vp, u32]
    lib.sdrfm_ring_submit.restype = C.c_int
    lib.sdrfm_ring_collect.argtypes = [vp, vp, u32, u32p, C.c_int]
    lib.sdrfm_ring_collect.restype = C.c_int
    lib.sdrfm_pcm_sink_create.argtypes = [u32, C.c_float, C.c_float, C.c_int32, C.POINTER(vp)]
    lib.sdrfm_pcm_sink_create.restype = C.c_int
    lib.sdrfm_pcm_sink_destroy.argtypes = [vp]
    lib.sdrfm_pcm_sink_destroy.restype = None
    lib.sdrfm_pcm_sink_reset.argtypes = [vp]
    lib.sdrfm_pcm_sink_reset.restype = C.c_int
    lib.sdrfm_pcm_sink_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, C.c_size_t, u32]
    lib.sdrfm_pcm_sink_process_batch.restype = C.c_int
    lib.sdrfm_pcm_sink_set_stream.argtypes = [vp, vp]
    lib.sdrfm_pcm_sink_set_stream.restype = C.c_int
    lib.sdrfm_pcm_sink_synchronize.argtypes = [vp]
    lib.sdrfm_pcm_sink_synchronize.restype = C.c_int
    lib.sdrfm_pcm_sink_get_state.argtypes = [vp, C.POINTER(C.c_float)]
    lib.sdrfm_pcm_sink_get_state.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_create.argtypes = [u32, C.c_float, C.c_float, C.c_int32, C.POINTER(vp)]
    lib.sdrfm_pcm_stereo_sink_create.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_destroy.argtypes = [vp]
    lib.sdrfm_pcm_stereo_sink_destroy.restype = None
    lib.sdrfm_pcm_stereo_sink_reset.argtypes = [vp]
    lib.sdrfm_pcm_stereo_sink_reset.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_process_batch.argtypes = [vp, vp, vp, C.c_size_t, u32, vp, C.c_size_t, u32]
    lib.sdrfm_pcm_stereo_sink_process_batch.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_set_stream.argtypes = [vp, vp]
    lib.sdrfm_pcm_stereo_sink_set_stream.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_synchronize.argtypes = [vp]
    lib.sdrfm_pcm_stereo_sink_synchronize.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_get_state.argtypes = [vp, C.POINTER(C.c_float)]
    lib.sdrfm_pcm_stereo_sink_get_state.restype = C.c_int
    lib.sdrfm_stereo_process_batch_pcm.argtypes = [vp, vp, vp, C.c_size_t, u32, vp, vp, C.c_size_t, vp, C.c_size_t, vp, u32p, u32]
    lib.sdrfm_stereo_process_batch_pcm.restype = C.c_int
    lib.sdrfm_bcast_process_batch_pcm.argtypes = [vp, vp, vp, C.c_size_t, u32, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, u32p, u32p, u32]
    lib.sdrfm_bcast_process_batch_pcm.restype = C.c_int
    lib.sdrfm_scan_create.argtypes = [C.POINTER(ScanConfig), C.POINTER(vp)]
    lib.sdrfm_scan_create.restype = C.c_int
    lib.sdrfm_scan_destroy.argtypes = [vp]
    lib.sdrfm_scan_destroy.restype = None
    lib.sdrfm_scan_reset.argtypes = [vp]
    lib.sdrfm_scan_reset.restype = C.c_int
    lib.sdrfm_scan_tune.argtypes = [vp, vp, vp]
    lib.sdrfm_scan_tune.restype = C.c_int
    lib.sdrfm_scan_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, u32]
    lib.sdrfm_scan_process_batch.restype = C.c_int
    lib.sdrfm_scan_set_stream.argtypes = [vp, vp]
    lib.sdrfm_scan_set_stream.restype = C.c_int
    lib.sdrfm_scan_synchronize.argtypes = [vp]
    lib.sdrfm_scan_synchronize.restype = C.c_int
    lib.sdrfm_scan_kernel_name.argtypes = [vp]
    lib.sdrfm_scan_kernel_name.restype = C.c_char_p
    lib.sdrfm_scan_report.argtypes = [vp, C.c_double, u32, C.c_double, C.POINTER(ScanReport)]
    lib.sdrfm_scan_report.restype = C.c_int
    lib.sdrfm_scan_meter_add.argtypes = [vp, vp]
    lib.sdrfm_scan_meter_add.restype = C.c_int
    lib.sdrfm_bcast_process_batch_metered.argtypes = [vp, vp, vp, C.c_size_t, u32, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, vp, u32p, u32p,
                                                      u32]
    lib.sdrfm_bcast_process_batch_metered.restype = C.c_int
    lib.sdrfm_bcast_retune.argtypes = [vp, vp, vp, vp, vp, u32]
    lib.sdrfm_bcast_retune.restype = C.c_int
    lib.sdrfm_bcast_set_audio.argtypes = [vp, vp, vp, u32]
    lib.sdrfm_bcast_set_audio.restype = C.c_int
    lib.sdrfm_bcast_get_audio.argtypes = [vp, vp, vp, vp, vp]
    lib.sdrfm_bcast_get_audio.restype = C.c_int
    lib.sdrfm_pcm_deemph_stereo_hicut_s16.argtypes = [vp, vp, u32, C.c_float, C.c_float, C.c_uint16, C.c_uint16, u32, u32, C.POINTER(C.c_float), vp]
    lib.sdrfm_pcm_deemph_stereo_hicut_s16.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_set_hicut.argtypes = [vp, vp, u32]
    lib.sdrfm_pcm_stereo_sink_set_hicut.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_get_hicut.argtypes = [vp, vp, vp, u32p]
    lib.sdrfm_pcm_stereo_sink_get_hicut.restype = C.c_int
    lib.sdrfm_scan_process_batch_hist.argtypes = [vp, vp, C.c_size_t, u32, vp, vp, C.c_size_t, u32]
    lib.sdrfm_scan_process_batch_hist.restype = C.c_int
    lib.sdrfm_scan_hist_add.argtypes = [vp, vp]
    lib.sdrfm_scan_hist_add.restype = C.c_int
    lib.sdrfm_scan_hist_report.argtypes = [vp, vp, C.c_double, u32, C.c_double, C.POINTER(ScanHistReport)]
    lib.sdrfm_scan_hist_report.restype = C.c_int
    lib.sdrfm_bcast_process_batch_metered_hist.argtypes = [vp, vp, vp, C.c_size_t, u32, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp,
                                                           C.c_size_t, u32p, u32p, u32]
    lib.sdrfm_bcast_process_batch_metered_hist.restype = C.c_int
    lib.sdrfm_bcast_hist_kernel_name.argtypes = [vp]
    lib.sdrfm_bcast_hist_kernel_name.restype = C.c_char_p
    lib.sdrfm_pcm_audio_meter_s16.argtypes = [vp, u32, u32, vp]
    lib.sdrfm_pcm_audio_meter_s16.restype = C.c_int
    lib.sdrfm_audio_meter_add.argtypes = [vp, vp]
    lib.sdrfm_audio_meter_add.restype = C.c_int
    lib.sdrfm_audio_meter_report.argtypes = [vp, C.c_double, C.POINTER(AudioReport)]
    lib.sdrfm_audio_meter_report.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_meter_enable.argtypes = [vp, u32]
    lib.sdrfm_pcm_stereo_sink_meter_enable.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_meter_disable.argtypes = [vp]
    lib.sdrfm_pcm_stereo_sink_meter_disable.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_meter_read.argtypes = [vp, vp, u32]
    lib.sdrfm_pcm_stereo_sink_meter_read.restype = C.c_int
    u64p = C.POINTER(C.c_uint64)
    lib.sdrfm_pcm_rate_create.argtypes = [C.POINTER(PcmRateConfig), C.POINTER(vp)]
    lib.sdrfm_pcm_rate_create.restype = C.c_int
    lib.sdrfm_pcm_rate_destroy.argtypes = [vp]
    lib.sdrfm_pcm_rate_destroy.restype = None
    lib.sdrfm_pcm_rate_reset.argtypes = [vp]
    lib.sdrfm_pcm_rate_reset.restype = C.c_int
    lib.sdrfm_pcm_rate_set_step.argtypes = [vp, vp]
    lib.sdrfm_pcm_rate_set_step.restype = C.c_int
    lib.sdrfm_pcm_rate_count.argtypes = [vp, u32, vp, u32p]
    lib.sdrfm_pcm_rate_count.restype = C.c_int
    lib.sdrfm_pcm_rate_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, C.c_size_t, vp, u32]
    lib.sdrfm_pcm_rate_process_batch.restype = C.c_int
    lib.sdrfm_pcm_rate_get_state.argtypes = [vp, vp, vp]
    lib.sdrfm_pcm_rate_get_state.restype = C.c_int
    lib.sdrfm_pcm_rate_set_stream.argtypes = [vp, vp]
    lib.sdrfm_pcm_rate_set_stream.restype = C.c_int
    lib.sdrfm_pcm_rate_synchronize.argtypes = [vp]
    lib.sdrfm_pcm_rate_synchronize.restype = C.c_int
    lib.sdrfm_pcm_rate_kernel_name.argtypes = [vp]
    lib.sdrfm_pcm_rate_kernel_name.restype = C.c_char_p
    lib.sdrfm_pcm_rate_s16.argtypes = [vp, u32, vp, u32, u32, C.c_uint64, u64p, vp, vp, u32, u32p]
    lib.sdrfm_pcm_rate_s16.restype = C.c_int
    lib.sdrfm_pcm_rate_check_coef.argtypes = [vp, u32, u32]
    lib.sdrfm_pcm_rate_check_coef.restype = C.c_int
    lib.sdrfm_pcm_limit_create.argtypes = [C.POINTER(PcmLimitConfig), C.POINTER(vp)]
    lib.sdrfm_pcm_limit_create.restype = C.c_int
    lib.sdrfm_pcm_limit_destroy.argtypes = [vp]
    lib.sdrfm_pcm_limit_destroy.restype = None
    lib.sdrfm_pcm_limit_reset.argtypes = [vp]
    lib.sdrfm_pcm_limit_reset.restype = C.c_int
    lib.sdrfm_pcm_limit_set_params.argtypes = [vp, vp, vp]
    lib.sdrfm_pcm_limit_set_params.restype = C.c_int
    lib.sdrfm_pcm_limit_set_gain.argtypes = [vp, vp, u32]
    lib.sdrfm_pcm_limit_set_gain.restype = C.c_int
    lib.sdrfm_pcm_limit_get_params.argtypes = [vp, vp, u32p]
    lib.sdrfm_pcm_limit_get_params.restype = C.c_int
    lib.sdrfm_pcm_limit_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, C.c_size_t, u32]
    lib.sdrfm_pcm_limit_process_batch.restype = C.c_int
    lib.sdrfm_pcm_limit_read.argtypes = [vp, vp, u32]
    lib.sdrfm_pcm_limit_read.restype = C.c_int
    lib.sdrfm_pcm_limit_get_state.argtypes = [vp, vp]
    lib.sdrfm_pcm_limit_get_state.restype = C.c_int
    lib.sdrfm_pcm_limit_set_stream.argtypes = [vp, vp]
    lib.sdrfm_pcm_limit_set_stream.restype = C.c_int
    lib.sdrfm_pcm_limit_synchronize.argtypes = [vp]
    lib.sdrfm_pcm_limit_synchronize.restype = C.c_int
    lib.sdrfm_pcm_limit_kernel_name.argtypes = [vp]
    lib.sdrfm_pcm_limit_kernel_name.restype = C.c_char_p
    lib.sdrfm_pcm_limit_s16.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, vp]
    lib.sdrfm_pcm_limit_s16.restype = C.c_int
    lib.sdrfm_pcm_limit_state_words.argtypes = [u32]
    lib.sdrfm_pcm_limit_state_words.restype = u32
    lib.sdrfm_pcm_limit_state_init.argtypes = [u32, vp]
    lib.sdrfm_pcm_limit_state_init.restype = C.c_int
    lib.sdrfm_pcm_limit_check_params.argtypes = [vp, u32, u32]
    lib.sdrfm_pcm_limit_check_params.restype = C.c_int
    lib.sdrfm_pcm_limit_add.argtypes = [vp, vp]
    lib.sdrfm_pcm_limit_add.restype = C.c_int
    lib.sdrfm_pcm_limit_report.argtypes = [vp, C.c_double, C.POINTER(PcmLimitReport)]
    lib.sdrfm_pcm_limit_report.restype = C.c_int
    lib.sdrfm_pcm_limit_ceiling.argtypes = [C.c_double]
    lib.sdrfm_pcm_limit_ceiling.restype = u32
    lib.sdrfm_pcm_tplimit_create.argtypes = [C.POINTER(PcmLimitConfig), vp, u32, u32, C.POINTER(vp)]
    lib.sdrfm_pcm_tplimit_create.restype = C.c_int
    lib.sdrfm_pcm_tplimit_get_detector.argtypes = [vp, u32p, u32p, u32p]
    lib.sdrfm_pcm_tplimit_get_detector.restype = C.c_int
    lib.sdrfm_pcm_tplimit_s16.argtypes = [vp, u32, u32, u32, u32, vp, vp, u32, u32, vp, vp, vp]
    lib.sdrfm_pcm_tplimit_s16.restype = C.c_int
    lib.sdrfm_pcm_tplimit_state_words.argtypes = [u32, u32]
    lib.sdrfm_pcm_tplimit_state_words.restype = u32
    lib.sdrfm_pcm_tplimit_state_init.argtypes = [u32, u32, vp]
    lib.sdrfm_pcm_tplimit_state_init.restype = C.c_int
    lib.sdrfm_pcm_tplimit_latency.argtypes = [u32, u32]
    lib.sdrfm_pcm_tplimit_latency.restype = u32
    lib.sdrfm_iq_meter_create.argtypes = [C.POINTER(IqMeterConfig), C.POINTER(vp)]
    lib.sdrfm_iq_meter_create.restype = C.c_int
    lib.sdrfm_iq_meter_destroy.argtypes = [vp]
    lib.sdrfm_iq_meter_destroy.restype = None
    lib.sdrfm_iq_meter_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, vp, u32]
    lib.sdrfm_iq_meter_process_batch.restype = C.c_int
    lib.sdrfm_iq_meter_set_stream.argtypes = [vp, vp]
    lib.sdrfm_iq_meter_set_stream.restype = C.c_int
    lib.sdrfm_iq_meter_synchronize.argtypes = [vp]
    lib.sdrfm_iq_meter_synchronize.restype = C.c_int
    lib.sdrfm_iq_meter_kernel_name.argtypes = [vp]
    lib.sdrfm_iq_meter_kernel_name.restype = C.c_char_p
    lib.sdrfm_iq_meter_u8.argtypes = [vp, C.c_size_t, vp, vp]
    lib.sdrfm_iq_meter_u8.restype = C.c_int
    lib.sdrfm_iq_meter_add.argtypes = [vp, vp]
    lib.sdrfm_iq_meter_add.restype = C.c_int
    lib.sdrfm_iq_hist_add.argtypes = [vp, vp]
    lib.sdrfm_iq_hist_add.restype = C.c_int
    lib.sdrfm_iq_meter_report.argtypes = [vp, C.POINTER(IqReport)]
    lib.sdrfm_iq_meter_report.restype = C.c_int
    lib.sdrfm_iq_hist_report.argtypes = [vp, C.POINTER(IqHistReport)]
    lib.sdrfm_iq_hist_report.restype = C.c_int
    lib.sdrfm_pcm_mix_create.argtypes = [C.POINTER(PcmMixConfig), vp, C.POINTER(vp)]
    lib.sdrfm_pcm_mix_create.restype = C.c_int
    lib.sdrfm_pcm_mix_destroy.argtypes = [vp]
    lib.sdrfm_pcm_mix_destroy.restype = None
    lib.sdrfm_pcm_mix_reset.argtypes = [vp]
    lib.sdrfm_pcm_mix_reset.restype = C.c_int
    lib.sdrfm_pcm_mix_set_routes.argtypes = [vp, vp, vp]
    lib.sdrfm_pcm_mix_set_routes.restype = C.c_int
    lib.sdrfm_pcm_mix_set_gains.argtypes = [vp, vp, u32]
    lib.sdrfm_pcm_mix_set_gains.restype = C.c_int
    lib.sdrfm_pcm_mix_get_slots.argtypes = [vp, vp, u32p]
    lib.sdrfm_pcm_mix_get_slots.restype = C.c_int
    lib.sdrfm_pcm_mix_process_batch.argtypes = [vp, vp, C.c_size_t, u32, vp, C.c_size_t, u32]
    lib.sdrfm_pcm_mix_process_batch.restype = C.c_int
    lib.sdrfm_pcm_mix_read.argtypes = [vp, vp, u32]
    lib.sdrfm_pcm_mix_read.restype = C.c_int
    lib.sdrfm_pcm_mix_set_stream.argtypes = [vp, vp]
    lib.sdrfm_pcm_mix_set_stream.restype = C.c_int
    lib.sdrfm_pcm_mix_synchronize.argtypes = [vp]
    lib.sdrfm_pcm_mix_synchronize.restype = C.c_int
    lib.sdrfm_pcm_mix_kernel_name.argtypes = [vp]
    lib.sdrfm_pcm_mix_kernel_name.restype = C.c_char_p
    lib.sdrfm_pcm_mix_s16.argtypes = [vp, C.c_size_t, u32, u32, vp, u32, u32, u32, vp, vp, vp]
    lib.sdrfm_pcm_mix_s16.restype = C.c_int
    lib.sdrfm_pcm_mix_check_slots.argtypes = [vp, u32, u32]
    lib.sdrfm_pcm_mix_check_slots.restype = C.c_int
    lib.sdrfm_pcm_mix_check_curve.argtypes = [vp]
    lib.sdrfm_pcm_mix_check_curve.restype = C.c_int
    lib.sdrfm_pcm_mix_add.argtypes = [vp, vp]
    lib.sdrfm_pcm_mix_add.restype = C.c_int
    lib.sdrfm_pcm_mix_report.argtypes = [vp, C.POINTER(PcmMixReport)]
    lib.sdrfm_pcm_mix_report.restype = C.c_int
    lib.sdrfm_loudness_default_coef.argtypes = [vp]
    lib.sdrfm_loudness_default_coef.restype = C.c_int
    lib.sdrfm_loudness_check_coef.argtypes = [vp]
    lib.sdrfm_loudness_check_coef.restype = C.c_int
    lib.sdrfm_loudness_check_domain.argtypes = [vp, vp, vp]
    lib.sdrfm_loudness_check_domain.restype = C.c_int
    lib.sdrfm_pcm_loudness_s16.argtypes = [vp, u32, vp, u32, vp, vp, u32, u32p]
    lib.sdrfm_pcm_loudness_s16.restype = C.c_int
    lib.sdrfm_loudness_gate_create.argtypes = [u32, C.POINTER(vp)]
    lib.sdrfm_loudness_gate_create.restype = C.c_int
    lib.sdrfm_loudness_gate_push.argtypes = [vp, vp, u32]
    lib.sdrfm_loudness_gate_push.restype = C.c_int
    lib.sdrfm_loudness_gate_report.argtypes = [vp, C.POINTER(LoudnessReport)]
    lib.sdrfm_loudness_gate_report.restype = C.c_int
    lib.sdrfm_loudness_gate_reset.argtypes = [vp]
    lib.sdrfm_loudness_gate_reset.restype = C.c_int
    lib.sdrfm_loudness_gate_free.argtypes = [vp]
    lib.sdrfm_loudness_gate_free.restype = None
    lib.sdrfm_pcm_stereo_sink_loudness_enable.argtypes = [vp, vp, u32, u32]
    lib.sdrfm_pcm_stereo_sink_loudness_enable.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_loudness_disable.argtypes = [vp]
    lib.sdrfm_pcm_stereo_sink_loudness_disable.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_loudness_read.argtypes = [vp, vp, u32, u64p, u32p, u32]
    lib.sdrfm_pcm_stereo_sink_loudness_read.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_loudness_get_state.argtypes = [vp, vp]
    lib.sdrfm_pcm_stereo_sink_loudness_get_state.restype = C.c_int
    u64 = C.c_uint64
    lib.sdrfm_truepeak_default_coef.argtypes = [vp, u32p, u32p]
    lib.sdrfm_truepeak_default_coef.restype = C.c_int
    lib.sdrfm_truepeak_check_coef.argtypes = [vp, u32, u32]
    lib.sdrfm_truepeak_check_coef.restype = C.c_int
    lib.sdrfm_truepeak_limit.argtypes = [C.c_double]
    lib.sdrfm_truepeak_limit.restype = u64
    lib.sdrfm_pcm_truepeak_s16.argtypes = [vp, u32, vp, u32, u32, u64, vp, vp]
    lib.sdrfm_pcm_truepeak_s16.restype = C.c_int
    lib.sdrfm_truepeak_add.argtypes = [vp, vp]
    lib.sdrfm_truepeak_add.restype = C.c_int
    lib.sdrfm_truepeak_report.argtypes = [vp, u32, C.c_double, C.POINTER(TruePeakReport)]
    lib.sdrfm_truepeak_report.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_truepeak_enable.argtypes = [vp, vp, u32, u32, u64]
    lib.sdrfm_pcm_stereo_sink_truepeak_enable.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_truepeak_disable.argtypes = [vp]
    lib.sdrfm_pcm_stereo_sink_truepeak_disable.restype = C.c_int
    lib.sdrfm_pcm_stereo_sink_truepeak_read.argtypes = [vp, vp, u32]
    lib.sdrfm_pcm_stereo_sink_truepeak_read.restype = C.c_int
    _libs[dev] = lib
    return lib
