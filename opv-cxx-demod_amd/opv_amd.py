"""ctypes binding of the C ABI in include/opv_demod.h (libopv_demod_hip.so).

Python is plumbing here (tests, bench, multi-GPU launch); the product is the shared library.
The directory name of this package contains a '-', so import it by path:

    import importlib.util, pathlib
    spec = importlib.util.spec_from_file_location("opv_amd", ".../opv-cxx-demod_amd/opv_amd.py")

or use ``load_opv_amd()`` from the repo-root ``__graft_entry__``.
There is no CPU fallback: if the library is missing or no MI355X is visible, calls raise.
"""
import ctypes as C
import os
import subprocess
import weakref
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("OPV_LIB", PKG / "libopv_demod_hip.so"))   # (OPV_LIB: dev switch, an experimental build of the same ABI)

SPS = 40
FRAME_BYTES = 134
FRAME_BITS = 1072
ENCODED_BITS = 2144
FRAME_SYMBOLS = 2168
CHUNK_SAMPLES = 86720
SAMPLE_RATE = 2168000.0

EXPORTS = [
    "opv_create", "opv_destroy", "opv_last_error", "opv_abi_version", "opv_push_iq", "opv_push_iq_batch", "opv_push_iq_batch_async", "opv_push_wait", "opv_flush",
    "opv_attach_device_iq", "opv_process", "opv_sync", "opv_set_frontend", "opv_reset_stream", "opv_pop_frames", "opv_pop_events",
    "opv_get_state", "opv_device_frames", "opv_hip_stream", "opv_comm_unique_id", "opv_comm_init", "opv_comm_init_all",
    "opv_comm_destroy", "opv_gather_frames", "opv_gather_frames_all", "opv_tap_soft", "opv_tap_chunks",
    "opv_tap_offset_energies", "opv_offset_ties_on_host", "opv_offset_ties_decided_on_host", "opv_offset_ties_left_to_device", "opv_tap_wave_info", "opv_tap_frontend_calls", "opv_tap_occupancy", "opv_decode_payloads", "opv_tx_bert_frame", "opv_tx_bert_frames", "opv_tx_modulated_samples",
    "opv_tx_modulate", "opv_tap_tx_checkpoints", "opv_frontend_kernel", "opv_channel_device", "opv_resample_device", "opv_enable_timing", "opv_kernel_times", "opv_tx_modulate_device", "opv_tx_modulate_device_to_host",
    "opv_export_size", "opv_export_streams", "opv_import_streams", "opv_blob_streams",
    "opv_wb_plan", "opv_wb_lo_table", "opv_wb_outputs", "opv_wb_create", "opv_wb_destroy", "opv_wb_push", "opv_wb_push_async", "opv_wb_push_device", "opv_wb_flush", "opv_tap_iq",
    "opv_wbr_plan", "opv_wbr_outputs", "opv_wb_create_rational",
    "opv_wb_seg_phase", "opv_wb_seg_next", "opv_wb_retune", "opv_wb_segments", "opv_wbtx_retune", "opv_wbtx_segments",
    "opv_tx_stream_create", "opv_tx_stream_reset", "opv_tx_stream_frames", "opv_tx_stream_tail", "opv_tx_stream_destroy", "opv_tap_tx_frame",
    "opv_tap_push_soft",
    "opv_enable_link_report", "opv_pop_frames_link", "opv_device_link", "opv_link_payloads",
    "opv_txb_create", "opv_txb_destroy", "opv_txb_reset", "opv_txb_get_state", "opv_txb_set_state", "opv_txb_round", "opv_txb_plan_round",
    "opv_tap_txb_patch",
    "opv_wbtx_plan", "opv_wbtx_create", "opv_wbtx_destroy", "opv_wbtx_push", "opv_wbtx_samples", "opv_wbtx_reset",
    "opv_wbtxr_plan", "opv_wbtxr_outputs", "opv_wbtx_create_rational",
    "opv_div_create", "opv_div_destroy", "opv_div_set_weights", "opv_div_round", "opv_div_pop_frames", "opv_div_get_state",
    "opv_div_tap_payload", "opv_div_match", "opv_div_earliest",
    "opv_scan_plan", "opv_scan_blocks", "opv_scan_create", "opv_scan_destroy", "opv_scan_push", "opv_scan_push_device", "opv_scan_pop",
    "opv_scan_reset", "opv_scan_carriers",
    "opv_push_iq_fmt", "opv_push_iq_batch_fmt", "opv_push_iq_batch_fmt_async", "opv_wb_push_fmt", "opv_wb_push_fmt_async", "opv_scan_push_fmt",
    "opv_convert_iq_device", "opv_iq_convert", "opv_iq_sample_bytes",
]

# typed IQ pushes (include/opv_demod.h, OPV_IQ_*): name -> (format code, numpy type of one component)
IQ_FORMATS = {"cs16": (0, np.int16), "cs8": (1, np.int8), "cu8": (2, np.uint8), "cf32": (3, np.float32)}


def _iq_block(fmt, block):
    """(format code, the block as a flat contiguous array of the format's component type - no copy if it is one already)"""
    if fmt not in IQ_FORMATS:
        raise OpvError(f"unknown sample format {fmt!r} (one of {', '.join(IQ_FORMATS)})")
    code, dtype = IQ_FORMATS[fmt]
    return code, np.ascontiguousarray(block, dtype).reshape(-1)


class OpvError(RuntimeError):
    pass


class Cfg(C.Structure):
    _fields_ = [("streaming", C.c_int32), ("have_init_offset", C.c_int32), ("init_offset_hz", C.c_double),
                ("afc_alpha", C.c_double), ("device", C.c_int32), ("coherent", C.c_int32),
                ("max_samples", C.c_uint64), ("pll_bw_hz", C.c_double)]


class WbCfg(C.Structure):
    _fields_ = [("decim", C.c_int32), ("n_channels", C.c_int32), ("n_taps", C.c_int32), ("out_shift", C.c_int32),
                ("first_sample", C.c_uint64)]


class WbrCfg(C.Structure):
    _fields_ = [("down", C.c_int32), ("up", C.c_int32), ("n_channels", C.c_int32), ("n_taps", C.c_int32), ("out_shift", C.c_int32),
                ("reserved", C.c_int32), ("first_sample", C.c_uint64)]


class WbtxCfg(C.Structure):
    _fields_ = [("interp", C.c_int32), ("n_channels", C.c_int32), ("n_taps", C.c_int32), ("out_shift", C.c_int32),
                ("first_sample", C.c_uint64)]


class WbtxrCfg(C.Structure):
    _fields_ = [("down", C.c_int32), ("up", C.c_int32), ("n_channels", C.c_int32), ("n_taps", C.c_int32), ("out_shift", C.c_int32),
                ("reserved", C.c_int32), ("first_sample", C.c_uint64)]


class WbSeg(C.Structure):
    """opv_wb_seg: a segment of a channel's LO schedule (32 bytes)"""
    _fields_ = [("start", C.c_uint64), ("phase", C.c_uint64), ("inc", C.c_uint64), ("ramp", C.c_int64)]

    def astuple(self):
        return (int(self.start), int(self.phase), int(self.inc), int(self.ramp))


class WbTune(C.Structure):
    """opv_wb_tune: an entry of a retune (40 bytes)"""
    _fields_ = [("channel", C.c_int32), ("phase_given", C.c_int32), ("at", C.c_uint64), ("centre_hz", C.c_double), ("rate_hz_s", C.c_double),
                ("phase", C.c_uint64)]


class ScanCfg(C.Structure):
    _fields_ = [("down", C.c_int32), ("up", C.c_int32), ("n_probes", C.c_int32), ("n_window", C.c_int32), ("hop", C.c_int32),
                ("n_avg", C.c_int32), ("out_shift", C.c_int32), ("ring_blocks", C.c_int32), ("first_sample", C.c_uint64)]


class ScanCarrier(C.Structure):
    _fields_ = [("centre_hz", C.c_double), ("excess", C.c_double), ("probe", C.c_int32), ("reserved", C.c_int32)]


class TxbState(C.Structure):
    _fields_ = [("symbols", C.c_uint64), ("sign_parity", C.c_int32), ("reserved", C.c_int32)]


TXB_MAX_RUN_FRAMES = 65536


class DivCfg(C.Structure):
    _fields_ = [("n_groups", C.c_int32), ("window", C.c_int32), ("normalise", C.c_int32), ("reserved", C.c_int32)]


class DivState(C.Structure):
    _fields_ = [("frames_emitted", C.c_uint32), ("frames_decoded", C.c_uint32), ("frames_perfect", C.c_uint32),
                ("records_lost", C.c_uint32), ("softs_lost", C.c_uint32), ("stalled", C.c_int32)]


class DivMeta(C.Structure):
    _fields_ = [("payload_symbol", C.c_uint64 * 8), ("members", C.c_uint32), ("summed", C.c_uint32),
                ("viterbi_metric", C.c_int32), ("sync_ok", C.c_int32), ("sync_quality", C.c_double)]


DIV_MAX_BRANCHES = 8
DIV_MAX_WINDOW = 64
DIV_ENDED = 0xFFFFFFFFFFFFFFFF


class FrameMeta(C.Structure):
    _fields_ = [("viterbi_metric", C.c_int32), ("sync_ok", C.c_int32), ("sync_quality", C.c_double),
                ("release_symbol", C.c_uint64), ("payload_symbol", C.c_uint64)]


class StreamState(C.Structure):
    _fields_ = [("freq_offset_hz", C.c_double), ("timing_freq", C.c_double), ("est_offset_hz", C.c_double),
                ("mu", C.c_double), ("total_symbols", C.c_uint64), ("total_samples", C.c_uint64),
                ("chunk_origin", C.c_uint64), ("sync_state", C.c_int32), ("frames_released", C.c_int32),
                ("frames_decoded", C.c_int32), ("frames_perfect", C.c_int32), ("n_chunks", C.c_int32),
                ("flushed", C.c_int32), ("events_dropped", C.c_uint32), ("edge_ties", C.c_uint32),
                ("stalled", C.c_int32), ("offset_ties", C.c_int32)]


EVENT_DTYPE = np.dtype(
    [("kind", "<i4"), ("count", "<i4"), ("sym_idx", "<u8"), ("corr", "<f8"), ("raw", "<f8")], align=True)
META_DTYPE = np.dtype([("viterbi_metric", "<i4"), ("sync_ok", "<i4"), ("sync_quality", "<f8"),
                       ("release_symbol", "<u8"), ("payload_symbol", "<u8")], align=True)
DIV_META_DTYPE = np.dtype([("payload_symbol", "<u8", (8,)), ("members", "<u4"), ("summed", "<u4"), ("viterbi_metric", "<i4"),
                           ("sync_ok", "<i4"), ("sync_quality", "<f8")], align=True)                 # opv_div_meta, 88 bytes
DIV_REC_DTYPE = np.dtype([("payload_symbol", "<u8"), ("sync_quality", "<f8"), ("sync_ok", "<i4"), ("reserved", "<i4")], align=True)
DIV_FRAME_DTYPE = np.dtype([("anchor", "<u8"), ("payload_symbol", "<u8", (8,)), ("members", "<u4"), ("reserved", "<u4")], align=True)
LINK_DTYPE = np.dtype([("valid", "<i4"), ("bit_errors", "<i4"), ("weak", "<i4"), ("nonfinite", "<i4"),
                       ("m1", "<f8"), ("m2", "<f8"), ("ma", "<f8")], align=True)          # opv_link, 40 bytes


def link_esn0_db(rec):
    """SNR in dB of the demodulator's SOFT OUTPUT from link records (LINK_DTYPE, one or an array): decision-directed amplitude
    ma and noise power m2 - ma^2, 10 log10(ma^2 / (2 (m2 - ma^2))). +inf where m2 <= ma^2 (no noise left after rounding), nan
    where valid == 0 or nonfinite > 0. It describes the soft symbols the decoder saw under that formula; it is NOT a
    calibrated channel Es/N0 (the front-end's soft symbols are not a matched filter's output)."""
    rec = np.asarray(rec)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ma2 = rec["ma"].astype(np.float64) ** 2
        noise = rec["m2"] - ma2
        db = 10.0 * np.log10(ma2 / (2.0 * noise))
    db = np.where(rec["m2"] <= ma2, np.inf, db)
    return np.where((rec["valid"] == 0) | (rec["nonfinite"] > 0), np.nan, db)


def build(force=False):
    """Compile the library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    if force or not LIB_PATH.exists():
        subprocess.run(["make", "-s", "-C", str(PKG), "-j8", "all"], check=True)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise OpvError(f"{LIB_PATH} is missing: run `make -C {PKG}` (there is no CPU fallback)")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7. Two HIP runtimes in one process do not
        # work ("No HIP GPUs are available" in whichever initialises second), and the dynamic loader
        # keys on the soname: whichever copy is loaded first serves both. When torch is present, let
        # it load first so that this library binds to the runtime torch was built for.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(str(LIB_PATH))
        L.opv_last_error.restype = C.c_char_p
        L.opv_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Cfg)]
        L.opv_destroy.argtypes = [C.c_void_p]
        L.opv_destroy.restype = None
        L.opv_push_iq.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_flush.argtypes = [C.c_void_p, C.c_int]
        L.opv_push_iq_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_push_iq_batch_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_push_wait.argtypes = [C.c_void_p]
        L.opv_attach_device_iq.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int]
        L.opv_process.argtypes = [C.c_void_p]
        L.opv_sync.argtypes = [C.c_void_p]
        L.opv_set_frontend.argtypes = [C.c_void_p, C.c_int]
        L.opv_frontend_kernel.restype = C.c_char_p
        L.opv_frontend_kernel.argtypes = [C.c_void_p]
        L.opv_reset_stream.argtypes = [C.c_void_p, C.c_int]
        L.opv_pop_frames.restype = C.c_long
        L.opv_pop_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        L.opv_pop_events.restype = C.c_long
        L.opv_pop_events.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_get_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(StreamState)]
        L.opv_device_frames.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.opv_hip_stream.restype = C.c_void_p
        L.opv_hip_stream.argtypes = [C.c_void_p]
        L.opv_comm_unique_id.argtypes = [C.c_char_p]
        L.opv_comm_init.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.opv_comm_init_all.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]
        L.opv_comm_destroy.restype = None
        L.opv_comm_destroy.argtypes = [C.c_void_p]
        L.opv_gather_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.opv_gather_frames_all.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.opv_tap_soft.restype = C.c_long
        L.opv_tap_soft.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t]
        L.opv_tap_push_soft.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_tap_chunks.restype = C.c_long
        L.opv_tap_chunks.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t]
        L.opv_tap_offset_energies.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.opv_tap_wave_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.opv_tap_frontend_calls.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.opv_offset_ties_on_host.argtypes = [C.c_void_p]
        L.opv_offset_ties_decided_on_host.restype = C.c_uint64
        L.opv_offset_ties_decided_on_host.argtypes = [C.c_void_p]
        L.opv_offset_ties_left_to_device.restype = C.c_uint64
        L.opv_offset_ties_left_to_device.argtypes = [C.c_void_p]
        L.opv_tap_occupancy.argtypes = [C.c_void_p, C.c_void_p]
        L.opv_decode_payloads.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_tx_bert_frame.restype = None
        L.opv_tx_bert_frame.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.opv_tx_bert_frames.restype = None
        L.opv_tx_bert_frames.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p]
        L.opv_tap_tx_checkpoints.restype = None
        L.opv_tap_tx_checkpoints.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p]
        L.opv_tx_modulated_samples.restype = C.c_size_t
        L.opv_tx_modulated_samples.argtypes = [C.c_size_t]
        L.opv_tx_modulate.restype = C.c_size_t
        L.opv_tx_modulate.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        L.opv_tap_tx_frame.restype = None
        L.opv_tap_tx_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_tx_stream_create.restype = C.c_void_p
        L.opv_tx_stream_create.argtypes = []
        L.opv_tx_stream_reset.restype = None
        L.opv_tx_stream_reset.argtypes = [C.c_void_p]
        L.opv_tx_stream_destroy.restype = None
        L.opv_tx_stream_destroy.argtypes = [C.c_void_p]
        L.opv_tx_stream_frames.restype = C.c_size_t
        L.opv_tx_stream_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.opv_tx_stream_tail.restype = C.c_size_t
        L.opv_tx_stream_tail.argtypes = [C.c_void_p]
        L.opv_channel_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                         C.c_double, C.c_uint64]
        L.opv_resample_device.restype = C.c_long
        L.opv_resample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_double]
        L.opv_enable_timing.argtypes = [C.c_void_p, C.c_int]
        L.opv_tx_modulate_device.restype = C.c_long
        L.opv_tx_modulate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.opv_kernel_times.argtypes = [C.c_void_p, C.c_void_p]
        L.opv_export_size.restype = C.c_size_t
        L.opv_export_size.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.opv_export_streams.restype = C.c_long
        L.opv_export_streams.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_import_streams.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_blob_streams.argtypes = [C.c_void_p, C.c_size_t]
        L.opv_wb_plan.argtypes = [C.POINTER(WbCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_wb_lo_table.restype = None
        L.opv_wb_lo_table.argtypes = [C.c_void_p]
        L.opv_wb_outputs.restype = C.c_size_t
        L.opv_wb_outputs.argtypes = [C.POINTER(WbCfg), C.c_uint64]
        L.opv_wb_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(WbCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_wb_destroy.restype = None
        L.opv_wb_destroy.argtypes = [C.c_void_p]
        L.opv_wb_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_wb_push_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_wb_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_wb_flush.argtypes = [C.c_void_p]
        L.opv_wbr_plan.argtypes = [C.POINTER(WbrCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_wbr_outputs.restype = C.c_size_t
        L.opv_wbr_outputs.argtypes = [C.POINTER(WbrCfg), C.c_uint64]
        L.opv_wb_create_rational.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(WbrCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_tap_iq.restype = C.c_long
        L.opv_tap_iq.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t]
        L.opv_enable_link_report.argtypes = [C.c_void_p, C.c_int]
        L.opv_pop_frames_link.restype = C.c_long
        L.opv_pop_frames_link.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.opv_device_link.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.opv_link_payloads.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.opv_txb_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int]
        L.opv_txb_destroy.restype = None
        L.opv_txb_destroy.argtypes = [C.c_void_p]
        L.opv_txb_reset.argtypes = [C.c_void_p, C.c_int]
        L.opv_txb_get_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(TxbState)]
        L.opv_txb_set_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(TxbState)]
        L.opv_txb_round.restype = C.c_long
        L.opv_txb_round.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.opv_txb_plan_round.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_tap_txb_patch.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p]
        L.opv_wb_seg_phase.restype = C.c_uint64
        L.opv_wb_seg_phase.argtypes = [C.POINTER(WbSeg), C.c_uint64]
        L.opv_wb_seg_next.argtypes = [C.POINTER(WbSeg), C.c_int32, C.c_int32, C.c_uint64, C.c_double, C.c_double, C.POINTER(WbSeg)]
        L.opv_wb_retune.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.opv_wb_segments.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_wbtx_retune.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.opv_wbtx_segments.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_wbtx_plan.argtypes = [C.POINTER(WbtxCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_wbtx_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(WbtxCfg), C.c_void_p, C.c_void_p]
        L.opv_wbtx_destroy.restype = None
        L.opv_wbtx_destroy.argtypes = [C.c_void_p]
        L.opv_wbtx_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.opv_wbtx_samples.restype = C.c_uint64
        L.opv_wbtx_samples.argtypes = [C.c_void_p]
        L.opv_wbtx_reset.argtypes = [C.c_void_p, C.c_uint64]
        L.opv_wbtxr_plan.argtypes = [C.POINTER(WbtxrCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_wbtxr_outputs.restype = C.c_uint64
        L.opv_wbtxr_outputs.argtypes = [C.POINTER(WbtxrCfg), C.c_uint64]
        L.opv_wbtx_create_rational.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(WbtxrCfg), C.c_void_p, C.c_void_p]
        L.opv_div_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(DivCfg), C.c_void_p, C.c_void_p]
        L.opv_div_destroy.restype = None
        L.opv_div_destroy.argtypes = [C.c_void_p]
        L.opv_div_set_weights.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.opv_div_round.argtypes = [C.c_void_p]
        L.opv_div_pop_frames.restype = C.c_long
        L.opv_div_pop_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.opv_div_get_state.argtypes = [C.c_void_p, C.c_int, C.POINTER(DivState)]
        L.opv_div_tap_payload.restype = C.c_long
        L.opv_div_tap_payload.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        L.opv_div_match.restype = C.c_long
        L.opv_div_match.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_div_earliest.restype = C.c_uint64
        L.opv_div_earliest.argtypes = [C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32]
        L.opv_scan_plan.argtypes = [C.POINTER(ScanCfg), C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_scan_blocks.restype = C.c_uint64
        L.opv_scan_blocks.argtypes = [C.POINTER(ScanCfg), C.c_uint64]
        L.opv_scan_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(ScanCfg), C.c_void_p, C.c_void_p]
        L.opv_scan_destroy.restype = None
        L.opv_scan_destroy.argtypes = [C.c_void_p]
        L.opv_scan_push.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_scan_push_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_scan_pop.restype = C.c_long
        L.opv_scan_pop.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
        L.opv_scan_reset.argtypes = [C.c_void_p, C.c_uint64]
        L.opv_scan_carriers.restype = C.c_long
        L.opv_scan_carriers.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_void_p, C.c_size_t]
        L.opv_push_iq_fmt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_push_iq_batch_fmt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_push_iq_batch_fmt_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.opv_wb_push_fmt.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_wb_push_fmt_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_scan_push_fmt.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.opv_convert_iq_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_iq_convert.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.opv_iq_sample_bytes.restype = C.c_size_t
        L.opv_iq_sample_bytes.argtypes = [C.c_int]
        _lib = L
    return _lib


def _chk(rc):
    if rc < 0:
        raise OpvError(f"opv error {rc}: {lib().opv_last_error().decode()}")
    return rc


def iq_convert(fmt, array):
    """opv_iq_convert: a block of `fmt` ("cs16", "cs8", "cu8", "cf32"; interleaved I, Q) as the int16 a typed push makes of it; host
    only, needs no device"""
    code, a = _iq_block(fmt, array)
    out = np.empty(a.size, np.int16)
    _chk(lib().opv_iq_convert(code, a.ctypes.data, out.ctypes.data, a.size // 2))
    return out


def comm_create(world, rank, device=0, uid=None):
    """RCCL communicator through the library's own binding (opv_comm_unique_id / opv_comm_init); returns (comm, uid)"""
    if uid is None:
        buf = C.create_string_buffer(128)
        _chk(lib().opv_comm_unique_id(buf))
        uid = buf.raw
    comm = C.c_void_p()
    _chk(lib().opv_comm_init(C.byref(comm), world, rank, uid, device))
    return comm, uid


def comm_init_all(devices):
    """opv_comm_init_all: one RCCL communicator per listed GPU inside THIS process (rank i on devices[i]); returns the list"""
    n = len(devices)
    comms = (C.c_void_p * n)()
    devs = (C.c_int * n)(*[int(d) for d in devices])
    _chk(lib().opv_comm_init_all(comms, n, devs))
    return [C.c_void_p(comms[i]) for i in range(n)]


def gather_frames_all(demods, comms, root, d_frames_all, d_counts_all):
    """opv_gather_frames_all: the gathers of every context of this process (demods[i] on comms[i]) in one RCCL group"""
    n = len(demods)
    ctxs = (C.c_void_p * n)(*[d.h.value for d in demods])
    cm = (C.c_void_p * n)(*[c.value for c in comms])
    _chk(lib().opv_gather_frames_all(ctxs, cm, n, root, C.c_void_p(d_frames_all), C.c_void_p(d_counts_all)))


def comm_destroy(comm):
    lib().opv_comm_destroy(comm)


# ---------------------------------------------------------------- transmit side (host)
def bert_frames(n, callsign="W5NYV", token=0xBBAADD, first=0):
    out = np.zeros((n, FRAME_BYTES), np.uint8)
    lib().opv_tx_bert_frames(callsign.encode(), token, first, n, out.ctypes.data)
    return out


def callsign_of(frame):
    """Base-40 station id of a 134-byte frame's first six bytes (what the reference prints as `Station ID`,
    ref src/opv-demod.cpp:907-925 / src/opv-mod.cpp:63-90: big-endian 48 bits, first character least significant)"""
    v = int.from_bytes(bytes(bytearray(frame[:6])), "big")
    out = ""
    while v:
        c = v % 40
        out += "?" if c == 0 else chr(64 + c) if c <= 26 else chr(48 + c - 27) if c <= 36 else "-/."[c - 37]
        v //= 40
    return out


def tx_checkpoints(first, count):
    """(ph1, ph2) of the modulator's NCOs at symbols 128 * (first .. first + count - 1) of a run (parity tap)"""
    out = np.empty((count, 2), np.float64)
    lib().opv_tap_tx_checkpoints(first, count, out.ctypes.data)
    return out


def modulate(frames):
    frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
    n = lib().opv_tx_modulated_samples(len(frames))
    iq = np.empty(2 * n, np.int16)
    w = lib().opv_tx_modulate(frames.ctypes.data, len(frames), iq.ctypes.data)
    assert w == n
    return iq


def tx_frame_taps(frame):
    """(randomised bytes, coded bits in encoder order, interleaved bits) of one 134-byte frame (opv_tap_tx_frame)"""
    frame = np.ascontiguousarray(frame, np.uint8).reshape(FRAME_BYTES)
    r, c, i = np.empty(FRAME_BYTES, np.uint8), np.empty(2144, np.uint8), np.empty(2144, np.uint8)
    lib().opv_tap_tx_frame(frame.ctypes.data, r.ctypes.data, c.ctypes.data, i.ctypes.data)
    return r, c, i


class TxStream:
    """the host modulator with its state carried from call to call (opv_tx_stream_*; reference HDLModulator,
    src/opv-mod.cpp:219-291)"""

    def __init__(self):
        self.h = lib().opv_tx_stream_create()
        if not self.h:
            raise OpvError("opv_tx_stream_create failed")

    def reset(self):
        lib().opv_tx_stream_reset(self.h)

    def frames(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
        iq = np.empty(2 * len(frames) * 2168 * 40, np.int16)
        w = lib().opv_tx_stream_frames(self.h, frames.ctypes.data, len(frames), iq.ctypes.data)
        assert w == iq.size // 2
        return iq

    @staticmethod
    def tail():
        iq = np.empty(2 * 4000, np.int16)
        assert lib().opv_tx_stream_tail(iq.ctypes.data) == 4000
        return iq

    def close(self):
        if self.h:
            lib().opv_tx_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- transmit bank (opv_txb_*)
def txb_plan_round(states, streams, n_frames, out_addr):
    """opv_txb_plan_round: what a round of a bank in `states` ((symbols, sign_parity) or (symbols, sign_parity, reserved) per
    stream) refuses (raises OpvError) or, if it holds, (first_block[count + 1], first_symbol[count]); host only, needs no device"""
    st = (TxbState * max(len(states), 1))(*[TxbState(*[int(v) for v in s]) for s in states])
    n = len(streams)
    ids = (C.c_int * max(n, 1))(*[int(s) for s in streams])
    nf = (C.c_size_t * max(n, 1))(*[int(v) for v in n_frames])
    addr = (C.c_size_t * max(n, 1))(*[int(v) for v in out_addr])                 # (uintptr_t)
    fb, fs = np.zeros(n + 1, np.uint32), np.zeros(max(n, 1), np.uint64)
    _chk(lib().opv_txb_plan_round(len(states), st, n, ids, nf, addr, fb.ctypes.data, fs.ctypes.data))
    return fb, fs[:n]


def txb_patch(symbol, sample, code):
    """opv_tap_txb_patch: int16 (I, Q) of one sample as a round's host patch evaluates it (libm); host only"""
    out = np.zeros(2, np.int16)
    _chk(lib().opv_tap_txb_patch(int(symbol), int(sample), int(code), out.ctypes.data))
    return out


class TxBank:
    """n_streams live modulators on the device of `demod`, their state carried from round to round (opv_txb_*,
    include/opv_demod.h). Close it before its Demod."""

    def __init__(self, demod, n_streams):
        self.demod = demod
        self.n_streams = int(n_streams)
        self.h = C.c_void_p()
        _chk(lib().opv_txb_create(C.byref(self.h), demod.h, self.n_streams))

    def round(self, streams, frames_list, d_out_ptrs, on_device=False):
        """opv_txb_round: stream streams[i] modulates frames_list[i] into the device pointer d_out_ptrs[i]. frames_list[i] is an
        array of 134-byte frames (host), or with on_device=True a pair (device pointer, number of frames). Returns the number
        of samples the host re-evaluated."""
        n = len(streams)
        keep = []
        if on_device:
            ptrs, counts = [int(p) for p, _ in frames_list], [int(k) for _, k in frames_list]
        else:
            keep = [np.ascontiguousarray(f, np.uint8).reshape(-1, FRAME_BYTES) for f in frames_list]
            ptrs, counts = [f.ctypes.data if len(f) else 0 for f in keep], [len(f) for f in keep]
        ids = (C.c_int * max(n, 1))(*[int(s) for s in streams])
        fp = (C.c_void_p * max(n, 1))(*ptrs)
        nf = (C.c_size_t * max(n, 1))(*counts)
        out = (C.c_void_p * max(n, 1))(*[int(p) for p in d_out_ptrs])
        return _chk(lib().opv_txb_round(self.h, n, ids, fp, nf, out, int(bool(on_device))))

    def state(self, stream):
        """(symbols, sign_parity) of one modulator"""
        s = TxbState()
        _chk(lib().opv_txb_get_state(self.h, int(stream), C.byref(s)))
        return int(s.symbols), int(s.sign_parity)

    def set_state(self, stream, symbols, sign_parity, reserved=0):
        s = TxbState(int(symbols), int(sign_parity), int(reserved))
        _chk(lib().opv_txb_set_state(self.h, int(stream), C.byref(s)))

    def reset(self, stream=-1):
        _chk(lib().opv_txb_reset(self.h, int(stream)))

    def close(self):
        if getattr(self, "h", None):
            lib().opv_txb_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def div_match(records, earliest, window=8, cursors=None, cap=None):
    """opv_div_match (host only, no device): records[b] = the frame records of branch b (DIV_REC_DTYPE, or a plain sequence of
    payload symbols), earliest[b] = E_b (DIV_ENDED: the branch has ended). Returns (group frames as DIV_FRAME_DTYPE, cursors)."""
    recs = []
    for r in records:
        r = np.asarray(r)
        if r.dtype != DIV_REC_DTYPE:
            q = np.zeros(len(r), DIV_REC_DTYPE)
            q["payload_symbol"] = r
            r = q
        recs.append(np.ascontiguousarray(r))
    nb = len(recs)
    ptrs = (C.c_void_p * max(nb, 1))(*[r.ctypes.data if len(r) else 0 for r in recs])
    n_recs = np.array([len(r) for r in recs], np.uint32)
    e = np.array([int(v) for v in earliest], np.uint64)
    cur = np.zeros(nb, np.uint32) if cursors is None else np.array(cursors, np.uint32)
    cap = int(n_recs.sum()) + 1 if cap is None else int(cap)
    out = np.zeros(cap, DIV_FRAME_DTYPE)
    n = _chk(lib().opv_div_match(nb, int(window), ptrs, n_recs.ctypes.data, e.ctypes.data, cur.ctypes.data, out.ctypes.data, cap))
    return out[:n].copy(), cur


def div_earliest(collecting, sync_state, anchor, next_symbol, ended=False):
    """opv_div_earliest: a branch's earliest possible future payload symbol off its tracker's carry (DIV_ENDED once it has ended)"""
    return int(lib().opv_div_earliest(int(collecting), int(sync_state), int(anchor), int(next_symbol), int(bool(ended))))


class Diversity:
    """Receive diversity over streams of `demod` (opv_div_*, include/opv_demod.h): groups = [[stream, ...], ...], 1..8 branch
    streams each, that carry the same transmission and are decoded as one. round() after demod.process(); close it before its
    Demod (one that outlives it answers OpvError -6)."""

    def __init__(self, demod, groups, window=8, normalise=False):
        self.demod = demod
        self.groups = [[int(s) for s in g] for g in groups]
        cfg = DivCfg(len(self.groups), int(window), int(bool(normalise)), 0)
        nb = (C.c_int * max(len(self.groups), 1))(*[len(g) for g in self.groups])
        flat = [s for g in self.groups for s in g]
        st = (C.c_int * max(len(flat), 1))(*flat)
        self.cap = int(demod.cfg.max_samples) // (FRAME_SYMBOLS * 38) + 8
        self.h = C.c_void_p()
        _chk(lib().opv_div_create(C.byref(self.h), demod.h, C.byref(cfg), nb, st))

    def round(self):
        """opv_div_round: match, combine and decode what the rounds launched so far have released; never waits"""
        _chk(lib().opv_div_round(self.h))

    def set_weights(self, group, w):
        w = np.ascontiguousarray(w, np.float64).reshape(-1)
        if w.size != len(self.groups[group]):
            raise OpvError("one weight per branch of the group")
        _chk(lib().opv_div_set_weights(self.h, int(group), w.ctypes.data))

    def pop_frames(self, group, link=False, cap=None):
        """(frames, meta as DIV_META_DTYPE); with link=True (frames, meta, link records as LINK_DTYPE)"""
        cap = cap or self.cap
        out = np.zeros((cap, FRAME_BYTES), np.uint8)
        meta = np.zeros(cap, DIV_META_DTYPE)
        rec = np.zeros(cap, LINK_DTYPE)
        n = _chk(lib().opv_div_pop_frames(self.h, int(group), out.ctypes.data, cap, meta.ctypes.data, rec.ctypes.data if link else None))
        return (out[:n].copy(), meta[:n].copy(), rec[:n].copy()) if link else (out[:n].copy(), meta[:n].copy())

    def state(self, group):
        s = DivState()
        _chk(lib().opv_div_get_state(self.h, int(group), C.byref(s)))
        return s

    def tap_payload(self, group, frame):
        """opv_div_tap_payload (parity tap): the 2144 combined soft symbols of group frame `frame`"""
        out = np.empty(ENCODED_BITS, np.float64)
        _chk(lib().opv_div_tap_payload(self.h, int(group), int(frame), out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().opv_div_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _blob_view(blob):
    """a blob as a contiguous uint8 array: bytes / bytearray / memoryview (a file, a socket) or an array"""
    if isinstance(blob, np.ndarray):
        return np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    return np.frombuffer(blob, np.uint8)


def blob_streams(blob):
    """opv_blob_streams: streams in an exported blob (host only: needs no device); raises on anything that is not one"""
    if blob is None:
        return _chk(lib().opv_blob_streams(None, 0))
    b = _blob_view(blob)
    return _chk(lib().opv_blob_streams(b.ctypes.data if b.size else None, b.size))


# ---------------------------------------------------------------- wideband front door (opv_wb_*)
def _wb_cfg(Cfg, centre_hz, taps, out_shift, first_sample, **ratio):
    """(cfg, centre, taps) for any of the four wideband configuration structs, every field by name: `ratio` is the kind's own
    (decim=, interp=, or down= and up=); a field not named (the rational structs' `reserved`) stays 0"""
    centre = np.ascontiguousarray(centre_hz, np.float64).reshape(-1)
    taps = np.ascontiguousarray(taps, np.int16).reshape(-1)
    cfg = Cfg(n_channels=centre.size, n_taps=taps.size, out_shift=int(out_shift), first_sample=int(first_sample),
              **{k: int(v) for k, v in ratio.items()})
    return cfg, centre, taps


def _wb_plan(plan, cfg, centre, taps):
    """one of the four opv_*_plan calls: validates a plan and returns its K phase increments (uint32)"""
    inc = np.zeros(max(centre.size, 1), np.uint32)
    _chk(plan(C.byref(cfg), centre.ctypes.data, taps.ctypes.data, inc.ctypes.data))
    return inc[:centre.size]


def wb_plan(decim, centre_hz, taps, out_shift, first_sample=0):
    """opv_wb_plan: validates a plan and returns its K phase increments (uint32); host only, needs no device"""
    return _wb_plan(lib().opv_wb_plan, *_wb_cfg(WbCfg, centre_hz, taps, out_shift, first_sample, decim=decim))


def wb_lo_table():
    """opv_wb_lo_table: T[i] = lrint(32767 cos(2 pi i / 4096)) as int16"""
    out = np.empty(4096, np.int16)
    lib().opv_wb_lo_table(out.ctypes.data)
    return out


def wb_outputs(decim, n_wide_total):
    """opv_wb_outputs: outputs per channel after n_wide_total wide samples, ceil(N / decim)"""
    cfg = WbCfg(int(decim), 1, 1, 0, 0)
    return int(lib().opv_wb_outputs(C.byref(cfg), int(n_wide_total)))


def wbr_plan(down, up, centre_hz, taps, out_shift, first_sample=0):
    """opv_wbr_plan: validates a plan of the rational door (wide rate 2 168 000 x down / up) and returns its K phase increments
    (uint32); host only, needs no device"""
    return _wb_plan(lib().opv_wbr_plan, *_wb_cfg(WbrCfg, centre_hz, taps, out_shift, first_sample, down=down, up=up))


def wbr_outputs(down, up, n_wide_total):
    """opv_wbr_outputs: outputs per channel after n_wide_total wide samples, ceil(N up / down)"""
    cfg = WbrCfg(int(down), int(up), 1, 1, 0, 0, 0)
    return int(lib().opv_wbr_outputs(C.byref(cfg), int(n_wide_total)))


# ---- the LO schedule of a channel (opv_wb_seg_*, opv_wb_retune, opv_wbtx_retune)
WB_TUNE_GAP, WB_TUNE_SEGS, WB_TUNE_MAX_RATE = 4096, 16, 1.0e7


def _wb_seg(seg):
    return seg if isinstance(seg, WbSeg) else WbSeg(*[int(v) for v in seg])


def wb_seg_phase(seg, a):
    """opv_wb_seg_phase: phi64(a) of a segment (a WbSeg or (start, phase, inc, ramp)); host only"""
    return int(lib().opv_wb_seg_phase(C.byref(_wb_seg(seg)), int(a) % (1 << 64)))


def wb_seg_next(prev, down, up, at, centre_hz, rate_hz_s=0.0):
    """opv_wb_seg_next: the WbSeg that follows `prev` from sample `at` on at centre_hz, moving by rate_hz_s; host only, needs no device"""
    out = WbSeg()
    _chk(lib().opv_wb_seg_next(C.byref(_wb_seg(prev)), int(down), int(up), int(at), float(centre_hz), float(rate_hz_s), C.byref(out)))
    return out


def _wb_tunes(tunes):
    """entries (channel, at, centre_hz[, rate_hz_s[, phase]]) or WbTune -> (count, array); a phase that is given is taken as is"""
    arr = (WbTune * max(len(tunes), 1))()
    for i, t in enumerate(tunes):
        if isinstance(t, WbTune):
            arr[i] = t
            continue
        t = tuple(t)
        arr[i] = WbTune(int(t[0]), int(len(t) > 4 and t[4] is not None), int(t[1]), float(t[2]), float(t[3]) if len(t) > 3 else 0.0,
                        int(t[4]) % (1 << 64) if len(t) > 4 and t[4] is not None else 0)
    return len(tunes), arr


def _wb_segments(call, h, channel):
    out = (WbSeg * WB_TUNE_SEGS)()
    n = _chk(call(h, int(channel), out, WB_TUNE_SEGS))
    return [WbSeg(*out[i].astuple()) for i in range(n)]


class Wideband:
    """A bank of DDCs on the device that feeds streams[k] of `demod` with the channel at centre_hz[k] of one wide capture
    (opv_wb_*, include/opv_demod.h). Close it before its Demod."""

    def __init__(self, demod, decim, streams, centre_hz, taps, out_shift, first_sample=0):
        self._create("Wideband", lib().opv_wb_create, demod, streams, _wb_cfg(WbCfg, centre_hz, taps, out_shift, first_sample, decim=decim))

    @classmethod
    def rational(cls, demod, down, up, streams, centre_hz, taps, out_shift, first_sample=0):
        """opv_wb_create_rational: the same object for a capture at 2 168 000 x down / up S/s (10 MS/s is 1250 / 271); `taps` is the
        prototype filter at up x that rate. push / push_async / push_device / flush / close are the ones below."""
        self = cls.__new__(cls)
        self._create("Wideband.rational", lib().opv_wb_create_rational, demod, streams, _wb_cfg(WbrCfg, centre_hz, taps, out_shift, first_sample, down=down, up=up))
        return self

    def _create(self, who, create, demod, streams, args):
        self.demod = demod
        self.cfg, centre, taps = args
        ids = (C.c_int * len(streams))(*[int(s) for s in streams])
        if len(streams) != centre.size:
            raise OpvError(f"{who}: one centre frequency per stream")
        self.h = C.c_void_p()
        _chk(create(C.byref(self.h), demod.h, C.byref(self.cfg), ids, centre.ctypes.data, taps.ctypes.data))
        self._inflight = []
        demod._wideband.add(self)

    def push(self, iq_wide, fmt="cs16"):
        """opv_wb_push; fmt other than "cs16": opv_wb_push_fmt, the block in the radio's own format"""
        if fmt != "cs16":
            code, iq = _iq_block(fmt, iq_wide)
            _chk(lib().opv_wb_push_fmt(self.h, code, iq.ctypes.data, iq.size // 2))
            return
        iq = np.ascontiguousarray(iq_wide, np.int16).reshape(-1)
        _chk(lib().opv_wb_push(self.h, iq.ctypes.data, iq.size // 2))

    def push_async(self, iq_wide, fmt="cs16"):
        """opv_wb_push_async: the block must stay alive and unchanged until demod.push_wait(). Several pushes may be in flight, so
        every block (or the copy made of it) is kept referenced here until then. fmt other than "cs16": opv_wb_push_fmt_async."""
        if fmt != "cs16":
            code, iq = _iq_block(fmt, iq_wide)
            self._inflight.append(iq)
            _chk(lib().opv_wb_push_fmt_async(self.h, code, iq.ctypes.data, iq.size // 2))
            return
        iq = np.ascontiguousarray(iq_wide, np.int16).reshape(-1)
        self._inflight.append(iq)
        _chk(lib().opv_wb_push_async(self.h, iq.ctypes.data, iq.size // 2))

    def push_device(self, dev_ptr, n_wide):
        _chk(lib().opv_wb_push_device(self.h, C.c_void_p(dev_ptr), int(n_wide)))

    def flush(self):
        _chk(lib().opv_wb_flush(self.h))

    def retune(self, tunes):
        """opv_wb_retune: `tunes` is a list of (channel, at, centre_hz[, rate_hz_s[, phase]]) or WbTune, `at` an absolute wide-sample
        index not yet pushed; the whole batch or nothing. Allowed between push_async calls."""
        n, arr = _wb_tunes(tunes)
        _chk(lib().opv_wb_retune(self.h, n, arr))

    def segments(self, channel):
        """opv_wb_segments: the channel's live segments (WbSeg), oldest first"""
        return _wb_segments(lib().opv_wb_segments, self.h, channel)

    def close(self):
        if getattr(self, "h", None):
            lib().opv_wb_destroy(self.h)                                     # (waits for the copy stream: nothing reads the blocks any more)
            self.h = C.c_void_p()
        self._inflight = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- wideband scan (opv_scan_*)
def _scan_cfg(down, up, probe_hz, window, hop, n_avg, out_shift, ring_blocks, first_sample):
    probes = np.ascontiguousarray(probe_hz, np.float64).reshape(-1)
    window = np.ascontiguousarray(window, np.int16).reshape(-1)
    cfg = ScanCfg(down=int(down), up=int(up), n_probes=probes.size, n_window=window.size, hop=int(hop), n_avg=int(n_avg),
                  out_shift=int(out_shift), ring_blocks=int(ring_blocks), first_sample=int(first_sample))
    return cfg, probes, window


def scan_plan(down, up, probe_hz, window, hop, n_avg, out_shift, ring_blocks=1, first_sample=0):
    """opv_scan_plan: validates a scan's plan and returns its P phase increments (uint32): wbr_plan's for the same (down, up,
    frequencies); host only, needs no device"""
    return _wb_plan(lib().opv_scan_plan, *_scan_cfg(down, up, probe_hz, window, hop, n_avg, out_shift, ring_blocks, first_sample))


def scan_blocks(n_window, hop, n_avg, n_wide_total, down=1, up=1):
    """opv_scan_blocks: blocks completed after n_wide_total wide samples, ((N - Lw) / H + 1) / A (0 while N < Lw)"""
    cfg = ScanCfg(int(down), int(up), 1, int(n_window), int(hop), int(n_avg), 0, 1, 0)
    return int(lib().opv_scan_blocks(C.byref(cfg), int(n_wide_total)))


def scan_carriers(row, f0_hz, step_hz, half_width_hz, ratio_q8, cap):
    """opv_scan_carriers: the carriers in one row of probe powers (or several rows added), probes at f0_hz + p step_hz; returns a
    list of (centre_hz, probe, excess), strongest first; host only"""
    row = np.ascontiguousarray(row, np.uint64).reshape(-1)
    out = (ScanCarrier * max(int(cap), 1))()
    n = _chk(lib().opv_scan_carriers(row.ctypes.data, row.size, float(f0_hz), float(step_hz), float(half_width_hz), int(ratio_q8), out, int(cap)))
    return [(out[i].centre_hz, out[i].probe, out[i].excess) for i in range(n)]


class Scan:
    """A bank of probes on the device of `demod`: the power of one wide capture at probe_hz[p], per block of n_avg windowed segments
    (opv_scan_*, include/opv_demod.h). Close it before its Demod."""

    def __init__(self, demod, down, up, probe_hz, window, hop, n_avg, out_shift, ring_blocks=16, first_sample=0):
        self.demod = demod
        self.cfg, probes, window = _scan_cfg(down, up, probe_hz, window, hop, n_avg, out_shift, ring_blocks, first_sample)
        self.h = C.c_void_p()
        _chk(lib().opv_scan_create(C.byref(self.h), demod.h, C.byref(self.cfg), probes.ctypes.data, window.ctypes.data))

    def push(self, iq_wide, fmt="cs16"):
        """opv_scan_push; fmt other than "cs16": opv_scan_push_fmt"""
        if fmt != "cs16":
            code, iq = _iq_block(fmt, iq_wide)
            _chk(lib().opv_scan_push_fmt(self.h, code, iq.ctypes.data, iq.size // 2))
            return
        iq = np.ascontiguousarray(iq_wide, np.int16).reshape(-1)
        _chk(lib().opv_scan_push(self.h, iq.ctypes.data, iq.size // 2))

    def push_device(self, dev_ptr, n_wide):
        _chk(lib().opv_scan_push_device(self.h, C.c_void_p(dev_ptr), int(n_wide)))

    def pop(self, cap=None):
        """opv_scan_pop: (rows uint64 [n][P], index of the first block); at most `cap` blocks (default: the ring)"""
        cap = self.cfg.ring_blocks if cap is None else int(cap)
        rows = np.zeros((cap, self.cfg.n_probes), np.uint64)
        first = C.c_uint64()
        n = _chk(lib().opv_scan_pop(self.h, rows.ctypes.data, cap, C.byref(first)))
        return rows[:n], int(first.value)

    def reset(self, first_sample=0):
        _chk(lib().opv_scan_reset(self.h, int(first_sample)))

    def close(self):
        if getattr(self, "h", None):
            lib().opv_scan_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- wideband transmit (opv_wbtx_*)
def wbtx_plan(interp, centre_hz, taps, out_shift, first_sample=0):
    """opv_wbtx_plan: validates a plan and returns its K phase increments (uint32); host only, needs no device"""
    return _wb_plan(lib().opv_wbtx_plan, *_wb_cfg(WbtxCfg, centre_hz, taps, out_shift, first_sample, interp=interp))


def wbtxr_plan(down, up, centre_hz, taps, out_shift, first_sample=0):
    """opv_wbtxr_plan: validates a plan of the rational up-converter bank (wide rate 2 168 000 x down / up) and returns its K phase
    increments (uint32): wbr_plan's for the same (down, up, centres); host only, needs no device"""
    return _wb_plan(lib().opv_wbtxr_plan, *_wb_cfg(WbtxrCfg, centre_hz, taps, out_shift, first_sample, down=down, up=up))


def wbtxr_outputs(down, up, n_in_total):
    """opv_wbtxr_outputs: wide samples written after n_in_total inputs per channel, ceil(N down / up)"""
    cfg = WbtxrCfg(int(down), int(up), 1, 1, 0, 0, 0)
    return int(lib().opv_wbtxr_outputs(C.byref(cfg), int(n_in_total)))


class WidebandTx:
    """A bank of up-converters on the device of `demod` that puts K per-channel captures (a TxBank's outputs) at centre_hz[k] of one
    wide capture (opv_wbtx_*, include/opv_demod.h). Close it before its Demod."""

    def __init__(self, demod, interp, centre_hz, taps, out_shift, first_sample=0):
        self._create(lib().opv_wbtx_create, demod, _wb_cfg(WbtxCfg, centre_hz, taps, out_shift, first_sample, interp=interp))

    @classmethod
    def rational(cls, demod, down, up, centre_hz, taps, out_shift, first_sample=0):
        """opv_wbtx_create_rational: the same object for a wide capture at 2 168 000 x down / up S/s (10 MS/s is 1250 / 271); `taps`
        is the prototype filter at down x 2 168 000 S/s. push / samples / reset / close are the ones below; a push behind N inputs
        writes wbtxr_outputs(down, up, N + n_in) - wbtxr_outputs(down, up, N) wide samples."""
        self = cls.__new__(cls)
        self._create(lib().opv_wbtx_create_rational, demod, _wb_cfg(WbtxrCfg, centre_hz, taps, out_shift, first_sample, down=down, up=up))
        return self

    def _create(self, create, demod, args):
        self.demod = demod
        self.cfg, centre, taps = args
        self.h = C.c_void_p()
        _chk(create(C.byref(self.h), demod.h, C.byref(self.cfg), centre.ctypes.data, taps.ctypes.data))

    def push(self, d_in_ptrs, n_in, d_out_ptr):
        """opv_wbtx_push: d_in_ptrs[k] is channel k's device pointer to n_in samples, or None for a channel absent from this push;
        n_in x interp wide samples go to the device pointer d_out_ptr (a rational object: the count `rational` names)"""
        if len(d_in_ptrs) != self.cfg.n_channels:
            raise OpvError("WidebandTx: one input pointer (or None) per channel")
        tab = (C.c_void_p * len(d_in_ptrs))(*[None if p is None else int(p) for p in d_in_ptrs])
        _chk(lib().opv_wbtx_push(self.h, tab, int(n_in), C.c_void_p(d_out_ptr)))

    def samples(self):
        """N: input samples per channel pushed since the object's creation or last reset"""
        return int(lib().opv_wbtx_samples(self.h))

    def reset(self, first_sample=0):
        _chk(lib().opv_wbtx_reset(self.h, int(first_sample)))

    def retune(self, tunes):
        """opv_wbtx_retune: as Wideband.retune; `at` is the absolute index of a wide sample not yet written"""
        n, arr = _wb_tunes(tunes)
        _chk(lib().opv_wbtx_retune(self.h, n, arr))

    def segments(self, channel):
        """opv_wbtx_segments: the channel's live segments (WbSeg), oldest first"""
        return _wb_segments(lib().opv_wbtx_segments, self.h, channel)

    def close(self):
        if getattr(self, "h", None):
            lib().opv_wbtx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- receiver
class Demod:
    """n_streams independent receivers on one GPU (mirrors the three reference objects
    MSKDemodulatorAFC + SyncTracker + FrameDecoder per stream)."""

    def __init__(self, n_streams=1, max_samples=1 << 22, streaming=True, init_offset=None, afc_alpha=0.001,
                 device=0, coherent=False, pll_bw=50.0):
        self.n_streams = n_streams
        self._wideband = weakref.WeakSet()      # Wideband objects feeding this context: push_wait releases their blocks too
        self.cfg = Cfg(int(streaming), int(init_offset is not None), float(init_offset or 0.0), afc_alpha,
                       device, int(coherent), int(max_samples), float(pll_bw))
        self.h = C.c_void_p()
        _chk(lib().opv_create(C.byref(self.h), n_streams, C.byref(self.cfg)))
        if os.environ.get("OPV_FRONTEND"):      # dev switch: run everything on one mapping (0 / 1 / 4 / 16)
            self.set_frontend(int(os.environ["OPV_FRONTEND"]))

    def close(self):
        if getattr(self, "h", None):
            lib().opv_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def push(self, stream, iq, fmt="cs16"):
        """opv_push_iq; fmt other than "cs16" ("cs8", "cu8", "cf32"): opv_push_iq_fmt, the block in the radio's own format"""
        if fmt != "cs16":
            code, a = _iq_block(fmt, iq)
            _chk(lib().opv_push_iq_fmt(self.h, stream, code, a.ctypes.data, a.size // 2))
            return
        iq = np.ascontiguousarray(iq, np.int16).reshape(-1)
        _chk(lib().opv_push_iq(self.h, stream, iq.ctypes.data, iq.size // 2))

    def push_batch(self, streams, blocks, wait=True, fmt="cs16"):
        """opv_push_iq_batch: blocks[i] (int16 IQ) goes to streams[i]; one wait for all copies. wait=False:
        opv_push_iq_batch_async - the blocks must stay alive and unchanged until push_wait() (they are kept referenced here).
        fmt other than "cs16": opv_push_iq_batch_fmt(_async), every block in that one format."""
        code, _ = IQ_FORMATS["cs16"] if fmt == "cs16" else _iq_block(fmt, [])
        blocks = [_iq_block(fmt, b)[1] for b in blocks]
        n = len(blocks)
        ids = (C.c_int * n)(*[int(s) for s in streams])
        ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in blocks])
        lens = (C.c_size_t * n)(*[b.size // 2 for b in blocks])
        typed = fmt != "cs16"
        if wait:
            _chk(lib().opv_push_iq_batch_fmt(self.h, code, n, ids, ptrs, lens) if typed else lib().opv_push_iq_batch(self.h, n, ids, ptrs, lens))
        else:
            held = getattr(self, "_inflight", None)        # the previous batch's blocks stay referenced until the call has waited for them
            _chk(lib().opv_push_iq_batch_fmt_async(self.h, code, n, ids, ptrs, lens) if typed else lib().opv_push_iq_batch_async(self.h, n, ids, ptrs, lens))
            self._inflight = blocks
            del held

    def convert_device(self, fmt, d_in, d_out, n_samples):
        """opv_convert_iq_device: n_samples of `fmt` at device address d_in to int16 at d_out, on the context's stream"""
        code, _ = _iq_block(fmt, [])
        _chk(lib().opv_convert_iq_device(self.h, code, C.c_void_p(d_in), C.c_void_p(d_out), int(n_samples)))

    def push_wait(self):
        _chk(lib().opv_push_wait(self.h))
        self._inflight = None
        for wb in self._wideband:
            wb._inflight = []

    def flush(self, stream):
        _chk(lib().opv_flush(self.h, stream))

    def attach(self, stream, dev_ptr, n_samples, eof=True):
        _chk(lib().opv_attach_device_iq(self.h, stream, C.c_void_p(dev_ptr), n_samples, int(eof)))

    def process(self):
        _chk(lib().opv_process(self.h))

    def sync(self):
        _chk(lib().opv_sync(self.h))

    def set_frontend(self, streams_per_wave):
        _chk(lib().opv_set_frontend(self.h, int(streams_per_wave)))

    def frontend_kernel(self):
        """name of the front-end kernel the last process() launched"""
        return lib().opv_frontend_kernel(self.h).decode()

    def reset(self, stream=-1):
        _chk(lib().opv_reset_stream(self.h, stream))

    def export_streams(self, streams):
        """opv_export_streams: a snapshot of the listed live streams as one self-describing blob (uint8 array) that
        import_streams of another context - same or other process, device or stream count - continues from"""
        ids = (C.c_int * len(streams))(*[int(s) for s in streams])
        cap = lib().opv_export_size(self.h, len(streams), ids)
        if cap == 0:
            raise OpvError(f"opv_export_size: {lib().opv_last_error().decode()}")
        blob = np.empty(cap, np.uint8)
        n = _chk(lib().opv_export_streams(self.h, len(streams), ids, blob.ctypes.data, cap))
        return blob[:n]

    def import_streams(self, dst_streams, blob):
        """opv_import_streams: blob's streams into the listed slots of this context (each reset first)"""
        b = _blob_view(blob)
        ids = (C.c_int * len(dst_streams))(*[int(s) for s in dst_streams])
        _chk(lib().opv_import_streams(self.h, len(dst_streams), ids, b.ctypes.data if b.size else None, b.size))

    def enable_timing(self, on=True):
        _chk(lib().opv_enable_timing(self.h, int(on)))

    def kernel_times(self):
        """ms of the last process(): dict(offset_search, msk_frontend, sync_track, frame_decode)"""
        t = (C.c_float * 4)()
        _chk(lib().opv_kernel_times(self.h, t))
        return dict(offset_search=t[0], msk_frontend=t[1], sync_track=t[2], frame_decode=t[3])

    def pop_frames(self, stream, cap=None, link=False):
        """(frames, meta); with link=True (opv_pop_frames_link; enable_link_report first) (frames, meta, link records)"""
        cap = cap or (int(self.cfg.max_samples) // (FRAME_SYMBOLS * 38) + 8)
        out = np.zeros((cap, FRAME_BYTES), np.uint8)
        meta = np.zeros(cap, META_DTYPE)
        if link:
            rec = np.zeros(cap, LINK_DTYPE)
            n = _chk(lib().opv_pop_frames_link(self.h, stream, out.ctypes.data, cap, meta.ctypes.data, rec.ctypes.data))
            return out[:n].copy(), meta[:n].copy(), rec[:n].copy()
        n = _chk(lib().opv_pop_frames(self.h, stream, out.ctypes.data, cap, meta.ctypes.data))
        return out[:n].copy(), meta[:n].copy()

    def enable_link_report(self, on=True):
        """opv_enable_link_report: per-frame link records (LINK_DTYPE) for every frame decoded from now on; off by default"""
        _chk(lib().opv_enable_link_report(self.h, int(on)))

    def device_link(self):
        """opv_device_link: device address of the [n_streams][frame_capacity] ring of opv_link records"""
        p = C.c_void_p()
        _chk(lib().opv_device_link(self.h, C.byref(p)))
        return p.value

    def link_payloads(self, soft):
        """opv_link_payloads: one link record per payload of 2144 soft symbols (stand-alone, like decode_payloads)"""
        soft = np.ascontiguousarray(soft, np.float64).reshape(-1, ENCODED_BITS)
        rec = np.zeros(len(soft), LINK_DTYPE)
        _chk(lib().opv_link_payloads(self.h, soft.ctypes.data, len(soft), rec.ctypes.data))
        return rec

    def pop_events(self, stream, cap=None):
        cap = cap or (4 * (int(self.cfg.max_samples) // (FRAME_SYMBOLS * 38) + 8) + 64)
        ev = np.zeros(cap, EVENT_DTYPE)
        n = _chk(lib().opv_pop_events(self.h, stream, ev.ctypes.data, cap))
        return ev[:n].copy()

    def state(self, stream):
        s = StreamState()
        _chk(lib().opv_get_state(self.h, stream, C.byref(s)))
        return s

    def soft(self, stream, first=0, cap=None):
        cap = cap or (int(self.cfg.max_samples) // 38 + 128)
        out = np.empty(cap, np.float64)
        n = _chk(lib().opv_tap_soft(self.h, stream, first, out.ctypes.data, cap))
        return out[:n].copy()

    def push_soft(self, stream, soft):
        """opv_tap_push_soft (parity tap): fp64 soft symbols appended to the stream's soft log as its front-end would have
        written them; the next process() runs the tracker and the decoder over them. Raises OpvError (-4) when the ring
        has no room, (-6) on a stream that has received IQ."""
        soft = np.ascontiguousarray(soft, np.float64).reshape(-1)
        _chk(lib().opv_tap_push_soft(self.h, stream, soft.ctypes.data, soft.size))

    def iq(self, stream, first=0, cap=None):
        """opv_tap_iq: the int16 IQ the stream's device buffer holds from absolute sample `first` on (interleaved)"""
        cap = cap or int(self.cfg.max_samples)
        out = np.empty(2 * cap, np.int16)
        n = _chk(lib().opv_tap_iq(self.h, stream, first, out.ctypes.data, cap))
        return out[:2 * n].copy()

    def chunks(self, stream, first=0):
        cap = int(self.cfg.max_samples) // 80000 + 4
        out = np.zeros((cap, 5), np.float64)
        n = _chk(lib().opv_tap_chunks(self.h, stream, first, out.ctypes.data, cap))
        return out[:n].copy()

    def offset_energies(self, stream):
        out = np.zeros(134, np.float64)
        _chk(lib().opv_tap_offset_energies(self.h, stream, out.ctypes.data))
        return out

    def offset_ties_on_host(self):
        """True when the offset search's near-ties are decided with the host's libm (include/opv_demod.h)"""
        return bool(lib().opv_offset_ties_on_host(self.h))

    def offset_ties_decided_on_host(self):
        """streams whose offset-search tie the host's libm has decided so far (final for a round after sync())"""
        return int(lib().opv_offset_ties_decided_on_host(self.h))

    def offset_ties_left_to_device(self):
        """streams listed for the host beyond what a round stages (their device decision stood); 0 in ordinary operation"""
        return int(lib().opv_offset_ties_left_to_device(self.h))

    def wave_info(self, stream):
        """(HW_ID, XCC_ID, shader cycles, 100 MHz ticks) of the wave that ran the stream's last front-end launch"""
        out = (C.c_uint64 * 4)()
        _chk(lib().opv_tap_wave_info(self.h, stream, out))
        return tuple(int(v) for v in out)

    def frontend_calls(self, stream):
        """(free, guarded): the stream's demodulate() calls since reset that ran without / with the timing clamp (opv_tap_frontend_calls)"""
        out = (C.c_uint64 * 2)()
        _chk(lib().opv_tap_frontend_calls(self.h, stream, out))
        return int(out[0]), int(out[1])

    def occupancy(self):
        """workgroups per CU the runtime can keep resident, per hot-path kernel (opv_tap_occupancy)"""
        out = (C.c_int * 6)()
        _chk(lib().opv_tap_occupancy(self.h, out))
        return dict(zip(("k_msk_frontend_rb", "k_msk_frontend_rb_wg4", "k_msk_frontend_x16_wg4", "k_msk_frontend_x4_wg4", "k_frame_decode",
                         "k_frame_scale"), [int(v) for v in out]))

    def decode_payloads(self, soft, taps=False):
        soft = np.ascontiguousarray(soft, np.float64).reshape(-1, ENCODED_BITS)
        n = len(soft)
        out = np.zeros((n, FRAME_BYTES), np.uint8)
        met = np.zeros(n, np.int32)
        q = np.zeros((n, ENCODED_BITS), np.int8) if taps else None
        de = np.zeros((n, ENCODED_BITS), np.int8) if taps else None
        bits = np.zeros((n, FRAME_BITS), np.uint8) if taps else None
        _chk(lib().opv_decode_payloads(self.h, soft.ctypes.data, n, out.ctypes.data, met.ctypes.data,
                                       q.ctypes.data if taps else None, de.ctypes.data if taps else None,
                                       bits.ctypes.data if taps else None))
        return dict(frames=out, metrics=met, q=q, deint=de, bits=bits)

    def device_frames(self):
        f, m, c, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        _chk(lib().opv_device_frames(self.h, C.byref(f), C.byref(m), C.byref(c), C.byref(cap)))
        return f.value, m.value, c.value, cap.value

    def hip_stream(self):
        return lib().opv_hip_stream(self.h)

    def gather_frames(self, comm, root, d_frames_all, d_counts_all):
        """opv_gather_frames: this context's frame buffer + counts to `root` over the RCCL communicator `comm`"""
        _chk(lib().opv_gather_frames(self.h, comm, root, C.c_void_p(d_frames_all), C.c_void_p(d_counts_all)))

    def modulate_device(self, frames, d_out):
        """TX chain into HBM (bit-identical to modulate()); returns samples re-evaluated on the host."""
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, FRAME_BYTES)
        return _chk(lib().opv_tx_modulate_device(self.h, frames.ctypes.data, len(frames), C.c_void_p(d_out)))

    def channel(self, d_in, d_out, n_samples, gain=1.0, f0_hz=0.0, sigma=0.0, seed=0):
        _chk(lib().opv_channel_device(self.h, C.c_void_p(d_in), C.c_void_p(d_out), n_samples, gain, f0_hz, sigma,
                                      seed))

    def resample(self, d_in, n_in, d_out, out_cap, clock_ppm):
        """opv_resample_device: returns the number of samples written to d_out"""
        n = lib().opv_resample_device(self.h, C.c_void_p(d_in), n_in, C.c_void_p(d_out), out_cap, clock_ppm)
        _chk(n)
        return n

    # convenience: the whole reference main() for one host capture on stream 0..n-1
    def receive(self, captures):
        """captures: list of int16 IQ arrays, one per stream. Returns per-stream dicts."""
        assert len(captures) == self.n_streams
        for s, iq in enumerate(captures):
            self.push(s, iq)
            self.flush(s)
        self.process()
        self.sync()
        res = []
        for s in range(self.n_streams):
            fr, meta = self.pop_frames(s)
            ev = self.pop_events(s)
            st = self.state(s)
            while st.stalled:                   # back-pressure: pop, run another round, until the stream has finished
                before = (st.total_symbols, st.frames_released, len(fr))
                self.process()
                f2, m2 = self.pop_frames(s)
                fr, meta = np.concatenate([fr, f2]), np.concatenate([meta, m2])
                ev = np.concatenate([ev, self.pop_events(s)])
                st = self.state(s)
                if st.stalled and (st.total_symbols, st.frames_released, len(fr)) == before:
                    raise OpvError(f"stream {s} stalled (0x{st.stalled:x}) without progress")
            res.append(dict(frames=fr, meta=meta, events=ev, soft=self.soft(s), state=st, chunks=self.chunks(s)))
        return res


def format_events(events):
    """The stderr lines of SyncTracker::process (reference src/opv-demod.cpp:651,677,695,699,705)."""
    lines = []
    for e in events:
        k, idx = int(e["kind"]), int(e["sym_idx"])
        if k == 1:
            lines.append("[%d] HUNTING→VERIFYING (corr=%.3f, raw=%.0f)" % (idx, e["corr"], e["raw"]))
        elif k == 2:
            lines.append("[%d] VERIFYING→LOCKED (frame %d)" % (idx, e["count"]))
        elif k == 3:
            lines.append("[%d] LOCKED: sync OK (corr=%.3f)" % (idx, e["corr"]))
        elif k == 4:
            lines.append("[%d] LOCKED: sync MISS #%d (corr=%.3f)" % (idx, e["count"], e["corr"]))
        elif k == 5:
            lines.append("[%d] LOCKED→HUNTING (lost lock)" % idx)
    return lines
