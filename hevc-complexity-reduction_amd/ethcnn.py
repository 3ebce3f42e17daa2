"""ctypes binding of libethcnn.so (include/ethcnn.h) -- the only way Python reaches the
HIP kernels.  No torch, no numpy math: numpy is used for buffers only.

There is deliberately no fallback: if the shared library is missing, or no gfx950 device
is usable, construction raises.
"""
import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libethcnn.so")
LIB_PATH = os.environ.get("ETHCNN_LIB", LIB_PATH)  # development knob: A/B builds of the same library

NOUT, NFEAT, NVEC, NFC2, SUB_BATCH = 21, 2688, 448, 336, 1024
BLOB_FLOATS = 1288210
LSTM_BLOB_FLOATS = 760078
LDP_BATCH_MAX, LDP_BATCH_BUNDLES = 32, 8  # sequences per LdpBatch call, bundles per LdpBatch

STAGES = ("tile", "trunk", "fc1", "heads", "gate")
DBG_FEATURES, DBG_FC1, DBG_FC2, DBG_LOGITS, DBG_RAW_PROBS = range(5)
_DBG_WIDTH = {DBG_FEATURES: NFEAT, DBG_FC1: NVEC, DBG_FC2: NFC2, DBG_LOGITS: NOUT, DBG_RAW_PROBS: NOUT}


ERR_ROWS_TIMEOUT, ERR_PLAN_REFUSED = -7, -8  # include/ethcnn.h
ERR_ARG, ERR_IO, ERR_FORMAT, ERR_DEVICE, ERR_NOWEIGHTS, ERR_NOMEM = -1, -2, -3, -4, -5, -6


def fast_plan_bound(blob, plan, lib=None):
    """a-priori floor bound of plan 2 / 3 on a probability for a blob in host memory (no device) -> (accepted_by_bound_alone, bound, feature_bound)"""
    lib = lib or load_library()
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    b, f = ctypes.c_double(), ctypes.c_double()
    rc = lib.ethcnn_fast_plan_bound(blob.ctypes.data, blob.size, int(plan), ctypes.byref(b), ctypes.byref(f))
    if rc not in (0, ERR_PLAN_REFUSED):
        raise EthCnnError(rc, "ethcnn_fast_plan_bound: bad arguments")
    return rc == 0, b.value, f.value


class EthCnnError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libethcnn error %d: %s" % (code, msg))
        self.code = code


class Options(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("max_ctus_per_pass", ctypes.c_int), ("host_threads", ctypes.c_int),
                ("reserved", ctypes.c_int * 5)]


class StageTimes(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_double * 5), ("launches", ctypes.c_int64 * 5), ("ctus", ctypes.c_int64),
                ("timed", ctypes.c_int64 * 5), ("timed_ctus", ctypes.c_int64 * 5), ("timing_errors", ctypes.c_int64)]


class CkptEntry(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("dtype", ctypes.c_int), ("rank", ctypes.c_int),
                ("shape", ctypes.c_int64 * 4), ("shard", ctypes.c_int), ("offset", ctypes.c_int64),
                ("size", ctypes.c_int64), ("crc32c", ctypes.c_uint32)]


class SourceFormat(ctypes.Structure):
    """ethcnn_source_format: what the file entries read (bit_depth 8..16; chroma_format 400 / 420 / 422 / 444)"""
    _fields_ = [("bit_depth", ctypes.c_int), ("chroma_format", ctypes.c_int)]


# every symbol include/ethcnn.h declares: name -> (restype, argtypes)
_vp, _cp, _i, _sz = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_size_t
_fp, _pd = ctypes.POINTER(ctypes.c_float), ctypes.c_ssize_t
SIGNATURES = {
    "ethcnn_create": (_i, [ctypes.POINTER(_vp), ctypes.POINTER(Options)]),
    "ethcnn_destroy": (None, [_vp]),
    "ethcnn_last_error": (_cp, [_vp]),
    "ethcnn_version": (_cp, []),
    "ethcnn_load_checkpoint": (_i, [_vp, _cp]),
    "ethcnn_load_blob": (_i, [_vp, _fp, _sz]),
    "ethcnn_load_synthetic": (_i, [_vp, ctypes.c_uint64, ctypes.c_double]),
    "ethcnn_get_blob": (_i, [_vp, _fp, _sz]),
    "ethcnn_model_name_for_qp": (_i, [_i, ctypes.c_char_p, _sz]),
    "ethcnn_load_thresholds": (_i, [_vp, _cp]),
    "ethcnn_parse_thresholds": (_i, [_cp, _fp, _fp]),
    "ethcnn_set_thresholds": (_i, [_vp, ctypes.c_float, ctypes.c_float]),
    "ethcnn_get_thresholds": (_i, [_vp, _fp, _fp]),
    "ethcnn_predict_luma_device": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _vp]),
    "ethcnn_narrow_rows_host": (_i, [_vp, _vp, _sz, _i]),
    "ethcnn_narrow_luma_device": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _vp, _pd, _pd]),
    "ethcnn_predict_luma16_device": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _i, _vp]),
    "ethcnn_predict_luma16": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _i, _fp]),
    "ethcnn_set_narrow_chunk": (_i, [_vp, _i]),
    "ethcnn_set_source_format": (_i, [_vp, _vp]),
    "ethcnn_get_source_format": (_i, [_vp, _vp]),
    "ethcnn_source_frame_bytes": (_i, [_vp, _i, _i, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "ethcnn_set_pass_pipeline": (_i, [_vp, _i]),
    "ethcnn_set_small_pass_launch": (_i, [_vp, _i]),
    "ethcnn_set_fc1_plan": (_i, [_vp, _i]),
    "ethcnn_get_fc1_plan": (_i, [_vp]),
    "ethcnn_check_fc1_plan": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "ethcnn_fast_plan_bound": (_i, [_vp, _sz, _i, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "ethcnn_measure_mfma_rate": (_i, [_vp, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]),
    "ethcnn_ldp_step": (_i, [_vp, _vp, _i, _i, _pd, _i, _i, _vp, _fp]),
    "ethcnn_ldp_get_state": (_i, [_vp, _fp, _sz]),
    "ethcnn_ldp_sequence_device": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _i, _vp, _vp]),
    "ethcnn_ldp_sequence": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _i, _vp, _fp]),
    "ethcnn_ldp_predict_yuv_file": (_i, [_vp, _cp, _i, _i, _i, _cp, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_ldp_set_sequence_chunk": (_i, [_vp, _i]),
    "ethcnn_ldp_sequence_bytes": (ctypes.c_int64, [_i, _i, _i, _i]),
    "ethcnn_ldp_group_create": (_i, [_vp, _i, ctypes.POINTER(_vp)]),
    "ethcnn_ldp_group_destroy": (None, [_vp]),
    "ethcnn_ldp_group_last_error": (_cp, [_vp]),
    "ethcnn_ldp_group_count": (_i, [_vp]),
    "ethcnn_ldp_group_load_lstm_checkpoint": (_i, [_vp, _i, _cp]),
    "ethcnn_ldp_group_load_lstm_blob": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_group_load_lstm_synthetic": (_i, [_vp, _i, ctypes.c_uint64, ctypes.c_double]),
    "ethcnn_ldp_group_get_lstm_blob": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_group_sequence_device": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, ctypes.POINTER(_i), _i, _vp, _vp]),
    "ethcnn_ldp_group_get_state": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_group_state_ctus": (ctypes.c_int64, [_vp, _i]),
    "ethcnn_ldp_group_set_chunk": (_i, [_vp, _i]),
    "ethcnn_ldp_group_bytes": (ctypes.c_int64, [_i, _i, _i, _i, _i]),
    "ethcnn_ldp_set_thresholds_group": (_i, [_vp, _i, ctypes.c_float, ctypes.c_float]),
    "ethcnn_ldp_clear_thresholds_group": (_i, [_vp, _i]),
    "ethcnn_ldp_get_thresholds_group": (_i, [_vp, _i, _fp, _fp, ctypes.POINTER(_i)]),
    "ethcnn_ldp_batch_create": (_i, [_vp, _i, ctypes.POINTER(_vp)]),
    "ethcnn_ldp_batch_destroy": (None, [_vp]),
    "ethcnn_ldp_batch_last_error": (_cp, [_vp]),
    "ethcnn_ldp_batch_bundles": (_i, [_vp]),
    "ethcnn_ldp_batch_load_lstm_checkpoint": (_i, [_vp, _i, _cp]),
    "ethcnn_ldp_batch_load_lstm_blob": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_batch_load_lstm_synthetic": (_i, [_vp, _i, ctypes.c_uint64, ctypes.c_double]),
    "ethcnn_ldp_batch_get_lstm_blob": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_batch_run_device": (_i, [_vp, _vp, _i]),
    "ethcnn_ldp_batch_get_state": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_batch_state_ctus": (ctypes.c_int64, [_vp, _i]),
    "ethcnn_ldp_batch_set_chunk": (_i, [_vp, _i]),
    "ethcnn_ldp_batch_bytes": (ctypes.c_int64, [ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), _i, _i]),
    "ethcnn_ldp_batch_plan": (_i, [ctypes.POINTER(_i), ctypes.POINTER(_i), _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), _i]),
    "ethcnn_ldp_set_thresholds_batch": (_i, [_vp, _i, ctypes.c_float, ctypes.c_float]),
    "ethcnn_ldp_clear_thresholds_batch": (_i, [_vp, _i]),
    "ethcnn_ldp_get_thresholds_batch": (_i, [_vp, _i, _fp, _fp, ctypes.POINTER(_i)]),
    "ethcnn_ldp_sessions_create": (_i, [_vp, _i, ctypes.POINTER(_vp)]),
    "ethcnn_ldp_sessions_destroy": (None, [_vp]),
    "ethcnn_ldp_sessions_last_error": (_cp, [_vp]),
    "ethcnn_ldp_sessions_bundles": (_i, [_vp]),
    "ethcnn_ldp_sessions_load_lstm_checkpoint": (_i, [_vp, _i, _cp]),
    "ethcnn_ldp_sessions_load_lstm_blob": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_sessions_load_lstm_synthetic": (_i, [_vp, _i, ctypes.c_uint64, ctypes.c_double]),
    "ethcnn_ldp_sessions_get_lstm_blob": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_sessions_open": (_i, [_vp, _i, _i, ctypes.POINTER(_i)]),
    "ethcnn_ldp_sessions_close": (_i, [_vp, _i]),
    "ethcnn_ldp_sessions_step_device": (_i, [_vp, _vp, _i]),
    "ethcnn_ldp_sessions_step": (_i, [_vp, _vp, _i]),
    "ethcnn_ldp_sessions_get_state": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_ldp_sessions_state_ctus": (ctypes.c_int64, [_vp, _i]),
    "ethcnn_ldp_sessions_bytes": (ctypes.c_int64, [ctypes.POINTER(_i), ctypes.POINTER(_i), _i]),
    "ethcnn_ldp_sessions_plan": (_i, [ctypes.POINTER(_i), _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), _i]),
    "ethcnn_ldp_sessions_set_thresholds": (_i, [_vp, _i, ctypes.c_float, ctypes.c_float]),
    "ethcnn_ldp_sessions_clear_thresholds": (_i, [_vp, _i]),
    "ethcnn_ldp_sessions_get_thresholds": (_i, [_vp, _i, _fp, _fp, ctypes.POINTER(_i)]),
    "ethcnn_ldp_step_begin": (_i, [_vp, _vp, _i, _i, _pd, _i, _i, _vp, _fp]),
    "ethcnn_rows_ready": (_i, [_vp, _i, _i]),
    "ethcnn_predict_luma_begin": (_i, [_vp, _vp, _i, _i, _i, _fp]),
    "ethcnn_predict_luma_end": (_i, [_vp]),
    "ethcnn_ldp_step_end": (_i, [_vp]),
    "ethcnn_host_alloc": (_i, [_vp, _sz, ctypes.POINTER(_vp)]),
    "ethcnn_host_free": (_i, [_vp, _vp]),
    "ethcnn_predict_luma": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _fp]),
    "ethcnn_predict_yuv_file": (_i, [_vp, _cp, _i, _i, _i, _cp, ctypes.POINTER(ctypes.c_int64)]),
    "ethcnn_predict_yuv_file_sharded": (_i, [_vp, ctypes.POINTER(ctypes.c_int), _i, _cp, _i, _i, _i, _cp, ctypes.POINTER(ctypes.c_int64)]),
    "ethcnn_shard_range": (_i, [ctypes.c_int64, _i, _i, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "ethcnn_get_startup_times": (_i, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "ethcnn_predict_yuv_shard": (_i, [_vp, _cp, _i, _i, _i, _cp, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_predict_yuv_range": (_i, [_vp, _cp, _i, _i, _i, _cp, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_ckpt_read_blob": (_i, [_cp, _fp, _sz, ctypes.c_char_p, _sz]),
    "ethcnn_resi_vectors_device":(_i, [_vp, _vp, _i, _i, _pd, _vp]),
    "ethcnn_resi_vectors": (_i, [_vp, _vp, _i, _i, _pd, _fp]),
    "ethcnn_load_lstm_checkpoint": (_i, [_vp, _cp]),
    "ethcnn_load_lstm_blob": (_i, [_vp, _fp, _sz]),
    "ethcnn_load_lstm_synthetic": (_i, [_vp, ctypes.c_uint64, ctypes.c_double]),
    "ethcnn_get_lstm_blob": (_i, [_vp, _fp, _sz]),
    "ethcnn_lstm_model_name_for_qp": (_i, [_i, ctypes.c_char_p, _sz]),
    "ethcnn_lstm_step_device": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ethcnn_ldp_predict_frame": (_i, [_vp, _vp, _i, _i, _pd, _i, _i, _vp, _fp, _fp]),
    "ethcnn_ckpt_read_lstm_blob": (_i, [_cp, _fp, _sz, ctypes.c_char_p, _sz]),
    "ethcnn_device_alloc": (_i, [_vp, _sz, ctypes.POINTER(_vp)]),
    "ethcnn_device_free": (_i, [_vp, _vp]),
    "ethcnn_memcpy_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "ethcnn_memcpy_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "ethcnn_synchronize": (_i, [_vp]),
    "ethcnn_device_name": (_i, [_vp, ctypes.c_char_p, _sz]),
    "ethcnn_set_profiling": (_i, [_vp, _i]),
    "ethcnn_get_stage_times": (_i, [_vp, ctypes.POINTER(StageTimes)]),
    "ethcnn_reset_stage_times": (_i, [_vp]),
    "ethcnn_debug_fetch": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_set_debug_capture": (_i, [_vp, _i]),
    "ethcnn_ckpt_read_index": (_i, [_cp, ctypes.POINTER(CkptEntry), _i, ctypes.POINTER(_i), ctypes.c_char_p, _sz]),
    "ethcnn_crc32c_masked": (ctypes.c_uint32, [_vp, _sz]),
    "ethcnn_host_thread_budget": (_i, [_i, _i]),
    "ethcnn_host_threads": (_i, [_vp]),
    "ethcnn_ckpt_write_blob": (_i, [_cp, _fp, _sz, ctypes.c_char_p, _sz]),
    "ethcnn_train_create": (_i, [_vp, ctypes.c_void_p, ctypes.POINTER(_vp)]),
    "ethcnn_train_destroy": (None, [_vp]),
    "ethcnn_train_init_weights": (_i, [_vp, ctypes.c_uint64]),
    "ethcnn_train_set_blob": (_i, [_vp, _fp, _fp, _sz]),
    "ethcnn_train_get_blob": (_i, [_vp, _fp, _fp, _sz]),
    "ethcnn_train_set_samples": (_i, [_vp, _i, _vp, _sz]),
    "ethcnn_train_set_qps": (_i, [_vp, ctypes.POINTER(ctypes.c_int), _i]),
    "ethcnn_train_run": (_i, [_vp, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_train_last_stats": (_i, [_vp, _fp, _fp]),
    "ethcnn_train_step_indices": (_i, [_vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int), _i, _fp, _fp]),
    "ethcnn_train_evaluate": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, _i, _fp, _fp, _fp]),
    "ethcnn_train_debug_fetch": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_train_last_error": (_cp, [_vp]),
    "ethcnn_train_group_check": (_i, [ctypes.c_void_p, _i, ctypes.c_char_p, _sz]),
    "ethcnn_train_group_create": (_i, [_vp, ctypes.c_void_p, _i, ctypes.POINTER(_vp)]),
    "ethcnn_train_group_destroy": (None, [_vp]),
    "ethcnn_train_group_init_weights": (_i, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "ethcnn_train_group_set_blob": (_i, [_vp, _i, _fp, _fp, _sz]),
    "ethcnn_train_group_get_blob": (_i, [_vp, _i, _fp, _fp, _sz]),
    "ethcnn_train_group_set_samples": (_i, [_vp, _i, _vp, _sz]),
    "ethcnn_train_group_set_samples_from": (_i, [_vp, _i, _vp, _i]),
    "ethcnn_train_group_set_qps": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int), _i]),
    "ethcnn_train_group_run": (_i, [_vp, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_train_group_last_stats": (_i, [_vp, _fp, _fp]),
    "ethcnn_train_group_step_indices": (_i, [_vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int), _i, _fp, _fp]),
    "ethcnn_train_group_evaluate": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, ctypes.POINTER(ctypes.c_int), _fp, _fp, _fp]),
    "ethcnn_train_group_debug_fetch": (_i, [_vp, _i, _i, _fp, _sz]),
    "ethcnn_train_group_last_error": (_cp, [_vp]),
    "ethcnn_ckpt_write_lstm_blob": (_i, [_cp, _fp, _sz, ctypes.c_char_p, _sz]),
    "ethcnn_lstm_train_create": (_i, [_vp, ctypes.c_void_p, ctypes.POINTER(_vp)]),
    "ethcnn_lstm_train_destroy": (None, [_vp]),
    "ethcnn_lstm_train_init_weights": (_i, [_vp, ctypes.c_uint64]),
    "ethcnn_lstm_train_set_blob": (_i, [_vp, _fp, _fp, _sz]),
    "ethcnn_lstm_train_get_blob": (_i, [_vp, _fp, _fp, _sz]),
    "ethcnn_lstm_train_set_qps": (_i, [_vp, ctypes.POINTER(ctypes.c_int), _i]),
    "ethcnn_lstm_train_set_samples": (_i, [_vp, _i, _vp, _sz]),
    "ethcnn_lstm_train_num_samples": (ctypes.c_int64, [_vp, _i]),
    "ethcnn_lstm_train_run": (_i, [_vp, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_lstm_train_last_stats": (_i, [_vp, _fp, _fp]),
    "ethcnn_lstm_train_step_indices": (_i, [_vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), _i, _fp, _fp]),
    "ethcnn_lstm_train_evaluate": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, _fp, _fp, _fp]),
    "ethcnn_lstm_train_debug_fetch": (_i, [_vp, _i, _fp, _sz]),
    "ethcnn_lstm_train_debug_rows": (ctypes.c_int64, [_vp]),
    "ethcnn_lstm_train_last_error": (_cp, [_vp]),
    "ethcnn_lstm_train_group_check": (_i, [ctypes.c_void_p, _i, ctypes.c_char_p, _sz]),
    "ethcnn_lstm_train_group_keep_list": (_i, [_vp, _sz, ctypes.POINTER(ctypes.c_int), _i, ctypes.POINTER(ctypes.c_int64),
                                               ctypes.POINTER(ctypes.c_int64)]),
    "ethcnn_lstm_train_group_create": (_i, [_vp, ctypes.c_void_p, _i, ctypes.POINTER(_vp)]),
    "ethcnn_lstm_train_group_destroy": (None, [_vp]),
    "ethcnn_lstm_train_group_init_weights": (_i, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "ethcnn_lstm_train_group_set_blob": (_i, [_vp, _i, _fp, _fp, _sz]),
    "ethcnn_lstm_train_group_get_blob": (_i, [_vp, _i, _fp, _fp, _sz]),
    "ethcnn_lstm_train_group_set_qps": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int), _i]),
    "ethcnn_lstm_train_group_set_samples": (_i, [_vp, _i, _vp, _sz]),
    "ethcnn_lstm_train_group_set_samples_from": (_i, [_vp, _i, _vp, _i]),
    "ethcnn_lstm_train_group_num_samples": (ctypes.c_int64, [_vp, _i, _i]),
    "ethcnn_lstm_train_group_run": (_i, [_vp, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_lstm_train_group_last_stats": (_i, [_vp, _fp, _fp]),
    "ethcnn_lstm_train_group_step_indices": (_i, [_vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32), _i, _fp, _fp]),
    "ethcnn_lstm_train_group_evaluate": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int32), ctypes.c_int64, _fp, _fp, _fp]),
    "ethcnn_lstm_train_group_debug_fetch": (_i, [_vp, _i, _i, _fp, _sz]),
    "ethcnn_lstm_train_group_debug_rows": (ctypes.c_int64, [_vp, _i]),
    "ethcnn_lstm_train_group_last_error": (_cp, [_vp]),
    "ethcnn_samples_create": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int), _i, _i, ctypes.c_uint64, ctypes.POINTER(_vp)]),
    "ethcnn_samples_destroy": (None, [_vp]),
    "ethcnn_samples_last_error": (_cp, [_vp]),
    "ethcnn_samples_add_sequence": (_i, [_vp, _i, _i, ctypes.POINTER(ctypes.c_char_p), _i, ctypes.POINTER(ctypes.c_char_p), _i]),
    "ethcnn_samples_set_source_format": (_i, [_vp, _vp]),
    "ethcnn_samples_cut16_device": (_i, [_vp, ctypes.POINTER(ctypes.c_int), _i, _i, _i, _i, _vp, _pd, _pd, _i, ctypes.POINTER(_vp), _vp,
                                         ctypes.c_int64]),
    "ethcnn_samples_count": (ctypes.c_int64, [_vp]),
    "ethcnn_samples_record_bytes": (_i, [_vp]),
    "ethcnn_samples_build": (_i, [_vp]),
    "ethcnn_samples_cut_device": (_i, [_vp, _i, ctypes.POINTER(ctypes.c_int), _i, _i, _i, _i, ctypes.POINTER(_vp), ctypes.POINTER(_pd),
                                       ctypes.POINTER(_pd), ctypes.POINTER(_vp), _i, _i, _vp, ctypes.c_int64]),
    "ethcnn_samples_read": (_i, [_vp, ctypes.c_int64, ctypes.c_int64, _i, ctypes.c_uint64, _vp]),
    "ethcnn_samples_write": (_i, [_vp, _cp, _i, ctypes.c_uint64]),
    "ethcnn_train_set_samples_from": (_i, [_vp, _i, _vp, _i]),
    "ethcnn_lstm_samples_plan": (_i, [_vp, _sz, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                      ctypes.POINTER(ctypes.c_int64)]),
    "ethcnn_lstm_samples_create": (_i, [_vp, ctypes.POINTER(ctypes.c_int), _i, _i, ctypes.c_uint64, ctypes.POINTER(_vp)]),
    "ethcnn_lstm_samples_destroy": (None, [_vp]),
    "ethcnn_lstm_samples_last_error": (_cp, [_vp]),
    "ethcnn_lstm_samples_build_from_set": (_i, [_vp, _vp]),
    "ethcnn_lstm_samples_build_from_records": (_i, [_vp, _vp, _sz]),
    "ethcnn_lstm_samples_count": (ctypes.c_int64, [_vp]),
    "ethcnn_lstm_samples_skipped": (ctypes.c_int64, [_vp]),
    "ethcnn_lstm_samples_read": (_i, [_vp, ctypes.c_int64, ctypes.c_int64, _vp]),
    "ethcnn_lstm_samples_write": (_i, [_vp, _cp]),
    "ethcnn_lstm_train_set_samples_from": (_i, [_vp, _i, _vp, _i]),
    "ethcnn_bench_lstm_repack": (_i, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, _vp]),
    "ethcnn_bench_lstm_gather": (_i, [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int64, _i, _vp]),
    "ethcnn_bench_copy": (_i, [_vp, _vp, _vp, _sz]),
    "ethcnn_calib_create": (_i, [_vp, ctypes.POINTER(_vp)]),
    "ethcnn_calib_destroy": (None, [_vp]),
    "ethcnn_calib_reset": (_i, [_vp]),
    "ethcnn_calib_add": (_i, [_vp, _vp, _vp, ctypes.c_int64]),
    "ethcnn_calib_add_device": (_i, [_vp, _vp, _vp, ctypes.c_int64]),
    "ethcnn_calib_add_frames": (_i, [_vp, _vp, _vp, _i, _i, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_calib_add_frames_device": (_i, [_vp, _vp, _vp, _i, _i, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_calib_get": (_i, [_vp, _vp, _vp, ctypes.POINTER(ctypes.c_uint64)]),
    "ethcnn_calib_choose": (_i, [_vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), _vp]),
    "ethcnn_calib_write_thr_info": (_i, [_cp, _vp, _i]),
    "ethcnn_sim_create": (_i, [_vp, ctypes.POINTER(_vp)]),
    "ethcnn_sim_destroy": (None, [_vp]),
    "ethcnn_sim_reset": (_i, [_vp]),
    "ethcnn_sim_add": (_i, [_vp, _vp, _vp, ctypes.c_int64]),
    "ethcnn_sim_add_device": (_i, [_vp, _vp, _vp, ctypes.c_int64]),
    "ethcnn_sim_add_frames": (_i, [_vp, _vp, _vp, _i, _i, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_sim_add_frames_device": (_i, [_vp, _vp, _vp, _i, _i, ctypes.c_int64, ctypes.c_int64]),
    "ethcnn_sim_info": (_i, [_vp, _vp]),
    "ethcnn_sim_eval": (_i, [_vp, _vp, ctypes.c_int64, _i, _vp]),
    "ethcnn_sim_sweep": (_i, [_vp, _vp, _i, _i, _vp]),
    "ethcnn_sim_search": (_i, [_vp, _vp, _i, _vp, ctypes.c_uint32, _i, _vp, _vp, ctypes.POINTER(_i)]),
    "ethcnn_sim_write_thr_info": (_i, [_cp, _vp, _i]),
    "ethcnn_decide_device": (_i, [_vp, _vp, _i, _i, ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp]),
    "ethcnn_decide": (_i, [_vp, _vp, _i, _i, ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp]),
    "ethcnn_decide_set_piece": (_i, [_vp, ctypes.c_int64]),
    "ethcnn_decide_frames_device": (_i, [_vp, _vp, _i, _i, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, _vp]),
    "ethcnn_decide_counts_from_codes": (_i, [_vp, ctypes.c_int64, _vp]),
    "ethcnn_budget_default_ladder": (_i, [_vp]),
    "ethcnn_budget_companion_thr": (_i, [_vp]),
    "ethcnn_budget_choose": (_i, [_vp, ctypes.c_int64, ctypes.c_int64, _vp, ctypes.c_uint32, _i, _vp, _vp, _vp, _vp]),
    "ethcnn_budget_cost": (_i, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp]),
    "ethcnn_budget_cost_device": (_i, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp]),
    "ethcnn_budget_bake_device": (_i, [_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp]),
    "ethcnn_budget_bake": (_i, [_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp]),
    "ethcnn_budget_control": (_i, [_vp, _vp, ctypes.c_int64, _vp, ctypes.c_uint32, _i, ctypes.c_int64, _i, _i, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "ethcnn_pacer_check": (_i, [_vp, ctypes.c_int64, _vp, ctypes.c_uint32, _i]),
    "ethcnn_pacer_create": (_i, [_vp, _vp, ctypes.c_int64, _vp, ctypes.c_uint32, _i, ctypes.POINTER(_vp)]),
    "ethcnn_pacer_destroy": (None, [_vp]),
    "ethcnn_pacer_reset": (_i, [_vp]),
    "ethcnn_pacer_frame_device": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ethcnn_pacer_frame": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ethcnn_pacer_last": (_i, [_vp, _vp]),
    "ethcnn_pacer_set_create": (_i, [_vp, _i, _vp, ctypes.c_int64, _vp, ctypes.c_uint32, _i, ctypes.POINTER(_vp)]),
    "ethcnn_pacer_set_destroy": (None, [_vp]),
    "ethcnn_pacer_set_slots": (_i, [_vp]),
    "ethcnn_pacer_set_launches": (ctypes.c_int64, [_vp]),
    "ethcnn_pacer_set_reset": (_i, [_vp, _i]),
    "ethcnn_pacer_set_frames_device": (_i, [_vp, _vp, _i]),
    "ethcnn_pacer_set_frames": (_i, [_vp, _vp, _i]),
    "ethcnn_pacer_set_last": (_i, [_vp, _i, _vp]),
    "ethcnn_pacer_set_plan": (_i, [_vp, _i, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ethcnn_pacer_policies_check": (_i, [_vp, _i, _vp, _i]),
    "ethcnn_pacer_policies_create": (_i, [_vp, _i, _vp, _i, _vp, ctypes.POINTER(_vp)]),
    "ethcnn_pacer_policies_count": (_i, [_vp]),
    "ethcnn_pacer_policies_of": (_i, [_vp, _i]),
    "ethcnn_pacer_policies_bind": (_i, [_vp, _i, _i]),
    "ethcnn_pacer_policies_plan": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ethcnn_ladder_check": (_i, [_vp, _i, ctypes.c_int64, ctypes.c_uint32]),
    "ethcnn_ladder_build": (_i, [_vp, _vp, _i, ctypes.c_int64, ctypes.c_uint32, _vp, _vp]),
    "ethcnn_ladder_thin": (_i, [_vp, ctypes.c_int64, ctypes.c_int64, _vp, _vp]),
    "ethcnn_ladder_write": (_i, [ctypes.c_char_p, _vp, ctypes.c_int64, _i]),
    "ethcnn_risk_set_reliability": (_i, [_vp, _vp]),
    "ethcnn_risk_eval": (_i, [_vp, _vp, ctypes.c_int64, _vp]),
    "ethcnn_risk_identity": (_i, [_vp]),
    "ethcnn_risk_from_hist": (_i, [_vp, _vp]),
    "ethcnn_risk_write": (_i, [ctypes.c_char_p, _vp]),
    "ethcnn_risk_read": (_i, [ctypes.c_char_p, _vp]),
    "ethcnn_risk_ladder_build": (_i, [_vp, _vp, _i, ctypes.c_int64, ctypes.c_uint64, _vp, _vp]),
    "ethcnn_reach_hist": (_i, [_vp, _vp, ctypes.c_int64, _i, _vp]),
    "ethcnn_reach_calibrate": (_i, [_vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), _i, _vp, _vp, _vp]),
    "ethcnn_compare_probs_device": (_i, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_float, _vp, _vp, _vp]),
    "ethcnn_compare_frames_device": (_i, [_vp, _vp, _vp, _i, _i, ctypes.c_int64, ctypes.c_float, _vp, _vp, _vp]),
    "ethcnn_compare_probs": (_i, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_float, _vp, _vp, _vp]),
    "ethcnn_compare_frames": (_i, [_vp, _vp, _vp, _i, _i, ctypes.c_int64, ctypes.c_float, _vp, _vp, _vp]),
    "ethcnn_audit_plan_bytes": (ctypes.c_int64, [_i, _i, _i]),
    "ethcnn_audit_plan_device": (_i, [_vp, _vp, _i, _i, _pd, _pd, _i, _i, _i, ctypes.c_float, _vp, _vp]),
    "ethcnn_audit_plan_yuv_file": (_i, [_vp, _cp, _i, _i, _i, _i, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, _vp, _vp]),
    "ethcnn_replay_plan": (_i, [_vp, _sz, _vp, _i, ctypes.POINTER(_i), _vp, ctypes.c_char_p, _sz]),
    "ethcnn_replay_uncut_device": (_i, [_vp, _vp, ctypes.c_int64, _vp, ctypes.c_int64, _i, _i, _i, _vp, _vp]),
    "ethcnn_replay_create": (_i, [_vp, ctypes.c_uint64, ctypes.POINTER(_vp)]),
    "ethcnn_replay_destroy": (None, [_vp]),
    "ethcnn_replay_last_error": (_cp, [_vp]),
    "ethcnn_replay_open_set": (_i, [_vp, _vp]),
    "ethcnn_replay_open_records": (_i, [_vp, _vp, _sz]),
    "ethcnn_replay_run_count": (_i, [_vp]),
    "ethcnn_replay_run_info": (_i, [_vp, _i, _vp]),
    "ethcnn_replay_set_chunk_frames": (_i, [_vp, _i]),
    "ethcnn_replay_run_bytes": (ctypes.c_int64, [_vp, _i, _i, _i]),
    "ethcnn_replay_run_device": (_i, [_vp, _i, _i, _vp, _vp]),
    "ethcnn_replay_run_group_bytes": (ctypes.c_int64, [_vp, _i, _i]),
    "ethcnn_replay_run_group_device": (_i, [_vp, _i, _i, ctypes.POINTER(_i), _vp, _vp, _vp]),
    "ethcnn_replay_feed_calib": (_i, [_vp, _i, _i, _vp]),
    "ethcnn_replay_feed_sim": (_i, [_vp, _i, _i, _vp]),
    "ethcnn_replay_batch_bytes": (ctypes.c_int64, [_vp, _vp, _i, ctypes.POINTER(_i)]),
    "ethcnn_replay_batch_device": (_i, [_vp, _vp, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), _vp, _vp]),
    "ethcnn_replay_batch_feed_calib": (_i, [_vp, _vp, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), _vp]),
    "ethcnn_replay_batch_feed_sim": (_i, [_vp, _vp, _i, ctypes.POINTER(_i), ctypes.POINTER(_i), ctypes.POINTER(_i), _vp]),
}

_lib = None


def load_library(path=None):
    """dlopen libethcnn.so and type every entry point.  Raises if it is not built."""
    global _lib
    if _lib is None or path is not None:
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise OSError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no fallback implementation)" % p)
        lib = ctypes.CDLL(p)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        if path is not None:
            return lib
        _lib = lib
    return _lib


def model_name_for_qp(qp):
    buf = ctypes.create_string_buffer(64)
    rc = load_library().ethcnn_model_name_for_qp(int(qp), buf, 64)
    if rc:
        raise EthCnnError(rc, "model_name_for_qp")
    return buf.value.decode()


def parse_thresholds(thr_info_path):
    a, b = ctypes.c_float(), ctypes.c_float()
    rc = load_library().ethcnn_parse_thresholds(os.fsencode(thr_info_path), ctypes.byref(a), ctypes.byref(b))
    if rc:
        raise EthCnnError(rc, "cannot parse %s" % thr_info_path)
    return a.value, b.value


def read_ckpt_index(index_path):
    """[(name, dtype, shape, shard, offset, size, masked_crc32c)] of a TF-V2 .index file."""
    lib = load_library()
    ents = (CkptEntry * 256)()
    n = ctypes.c_int(0)
    err = ctypes.create_string_buffer(400)
    rc = lib.ethcnn_ckpt_read_index(index_path.encode(), ents, 256, ctypes.byref(n), err, 400)
    if rc:
        raise EthCnnError(rc, err.value.decode("utf-8", "replace"))
    # (names come from a file: a corrupted key need not be UTF-8 -- found by tests/test_ckpt.py's byte-flip fuzz)
    return [(e.name.decode("utf-8", "replace"), e.dtype, tuple(e.shape[i] for i in range(e.rank)), e.shard, e.offset, e.size, e.crc32c)
            for e in ents[: n.value]]


def lstm_model_name_for_qp(qp):
    buf = ctypes.create_string_buffer(64)
    rc = load_library().ethcnn_lstm_model_name_for_qp(int(qp), buf, 64)
    if rc:
        raise EthCnnError(rc, "lstm_model_name_for_qp")
    return buf.value.decode()


def read_ckpt_lstm_blob(prefix):
    """ETH-LSTM TF-V2 bundle -> float32[LSTM_BLOB_FLOATS] in checkpoint layout (crc32c-checked, host only)."""
    out = np.empty(LSTM_BLOB_FLOATS, dtype=np.float32)
    err = ctypes.create_string_buffer(400)
    rc = load_library().ethcnn_ckpt_read_lstm_blob(os.fsencode(prefix), out.ctypes.data_as(_fp), out.size, err, 400)
    if rc:
        raise EthCnnError(rc, err.value.decode("utf-8", "replace"))
    return out


def write_ckpt_blob(prefix, blob):
    """float32[BLOB_FLOATS] -> <prefix>.index + <prefix>.data-00000-of-00001 (TF-V2 bundle, host only)"""
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    err = ctypes.create_string_buffer(400)
    rc = load_library().ethcnn_ckpt_write_blob(os.fsencode(prefix), blob.ctypes.data_as(_fp), blob.size, err, 400)
    if rc:
        raise EthCnnError(rc, err.value.decode("utf-8", "replace") or "ethcnn_ckpt_write_blob: bad arguments")


def write_ckpt_lstm_blob(prefix, blob):
    """float32[LSTM_BLOB_FLOATS] -> the ETH-LSTM TF-V2 bundle ethcnn_load_lstm_checkpoint restores (host only)"""
    blob = np.ascontiguousarray(blob, dtype=np.float32)
    err = ctypes.create_string_buffer(400)
    rc = load_library().ethcnn_ckpt_write_lstm_blob(os.fsencode(prefix), blob.ctypes.data_as(_fp), blob.size, err, 400)
    if rc:
        raise EthCnnError(rc, err.value.decode("utf-8", "replace") or "ethcnn_ckpt_write_lstm_blob: bad arguments")


def read_ckpt_blob(prefix):
    """TF-V2 bundle -> float32[BLOB_FLOATS] in checkpoint layout (crc32c-checked, host only)."""
    out = np.empty(BLOB_FLOATS, dtype=np.float32)
    err = ctypes.create_string_buffer(400)
    rc = load_library().ethcnn_ckpt_read_blob(os.fsencode(prefix), out.ctypes.data_as(_fp), out.size, err, 400)
    if rc:
        raise EthCnnError(rc, err.value.decode("utf-8", "replace"))
    return out


def crc32c_masked(data):
    b = bytes(data)
    return load_library().ethcnn_crc32c_masked(b, len(b))


def host_thread_budget(local_workers=1, usable_cpus=0):
    """staging-fill threads ONE predictor process starts when `local_workers` of them share the node (no device needed)"""
    return load_library().ethcnn_host_thread_budget(int(local_workers), int(usable_cpus))


def ldp_sequence_bytes(width, height, nframes, chunk_frames=0):
    """device bytes an ldp_sequence call holds for that chunk size (ethcnn_ldp_sequence_bytes; host only); negative = bad arguments"""
    return int(load_library().ethcnn_ldp_sequence_bytes(int(width), int(height), int(nframes), int(chunk_frames)))


def _int_array(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int * max(len(vals), 1))(*vals)


def ldp_batch_bytes(widths, heights, nframes, chunk_frames=0):
    """device bytes an LdpBatch.run_device call over sequences of these sizes and frame counts holds for that chunk size
    (ethcnn_ldp_batch_bytes; host only), the bundle images apart; negative for bad arguments"""
    if not (len(widths) == len(heights) == len(nframes)):
        raise ValueError("ldp_batch_bytes takes one width, height and frame count per sequence")
    return int(load_library().ethcnn_ldp_batch_bytes(_int_array(widths), _int_array(heights), _int_array(nframes), len(widths), int(chunk_frames)))


def ldp_batch_plan(nctus, nframes, chunk_frames=0):
    """the chunks of an LdpBatch.run_device call over sequences of these CTU and frame counts (ethcnn_ldp_batch_plan; host only) ->
    {"chunk_frames": Fc, "chunks": [{"members", "blocks": (level 16, level 32, level 64)}]}; raises EthCnnError for bad arguments"""
    if len(nctus) != len(nframes):
        raise ValueError("ldp_batch_plan takes one CTU count and one frame count per sequence")
    lib = load_library()
    fc, nchunks = ctypes.c_int(0), ctypes.c_int(0)
    args = (_int_array(nctus), _int_array(nframes), len(nctus), int(chunk_frames))
    rc = lib.ethcnn_ldp_batch_plan(*args, ctypes.byref(fc), ctypes.byref(nchunks), None, 0)
    if rc:
        raise EthCnnError(rc, "ethcnn_ldp_batch_plan: bad arguments")
    rows = (ctypes.c_int * (4 * max(nchunks.value, 1)))()
    rc = lib.ethcnn_ldp_batch_plan(*args, ctypes.byref(fc), ctypes.byref(nchunks), rows, nchunks.value)
    if rc:
        raise EthCnnError(rc, "ethcnn_ldp_batch_plan: bad arguments")
    return {"chunk_frames": fc.value,
            "chunks": [{"members": rows[4 * t], "blocks": (rows[4 * t + 1], rows[4 * t + 2], rows[4 * t + 3])} for t in range(nchunks.value)]}


def ldp_sessions_bytes(widths, heights):
    """device bytes the sessions of these picture sizes hold when they step together (ethcnn_ldp_sessions_bytes; host only), the bundle
    images apart; negative for bad arguments"""
    if len(widths) != len(heights):
        raise ValueError("ldp_sessions_bytes takes one width and one height per session")
    return int(load_library().ethcnn_ldp_sessions_bytes(_int_array(widths), _int_array(heights), len(widths)))


def ldp_sessions_plan(nctus, max_ctus_per_pass=0):
    """the layout of an LdpSessions step over pictures of these CTU counts, in this order (ethcnn_ldp_sessions_plan; host only) ->
    {"first_group": [...], "pass_groups": [...]}: picture j owns the 16-CTU groups from first_group[j] on, pass p holds pass_groups[p]
    groups; raises EthCnnError for bad arguments"""
    lib = load_library()
    first, npasses = (ctypes.c_int * max(len(nctus), 1))(), ctypes.c_int(0)
    args = (_int_array(nctus), len(nctus), int(max_ctus_per_pass), first, ctypes.byref(npasses))
    rc = lib.ethcnn_ldp_sessions_plan(*args, None, 0)
    if rc:
        raise EthCnnError(rc, "ethcnn_ldp_sessions_plan: bad arguments")
    passes = (ctypes.c_int * max(npasses.value, 1))()
    rc = lib.ethcnn_ldp_sessions_plan(*args, passes, npasses.value)
    if rc:
        raise EthCnnError(rc, "ethcnn_ldp_sessions_plan: bad arguments")
    return {"first_group": [first[j] for j in range(len(nctus))], "pass_groups": [passes[p] for p in range(npasses.value)]}


def ldp_group_bytes(width, height, nframes, chunk_frames=0, k=1):
    """device bytes an LdpGroup.sequence_device call of k members holds for that chunk size (ethcnn_ldp_group_bytes; host only), the
    k bundle images apart; negative = bad arguments"""
    return int(load_library().ethcnn_ldp_group_bytes(int(width), int(height), int(nframes), int(chunk_frames), int(k)))


def source_frame_bytes(width, height, bit_depth=8, chroma=420):
    """(luma_bytes, frame_bytes) of a planar frame in that source format (ethcnn_source_frame_bytes; host only)"""
    fmt = SourceFormat(int(bit_depth), int(chroma))
    a, b = ctypes.c_int64(), ctypes.c_int64()
    rc = load_library().ethcnn_source_frame_bytes(ctypes.addressof(fmt), int(width), int(height), ctypes.byref(a), ctypes.byref(b))
    if rc:
        raise EthCnnError(rc, "source_frame_bytes: no %dx%d frame of whole planes at %d bits, chroma format %d" % (width, height, bit_depth, chroma))
    return a.value, b.value


def narrow_rows_host(src16, bit_depth):
    """uint16 samples -> uint8 min(s >> (bit_depth - 8), 255), the narrowing rule of include/ethcnn.h on the host (no device)"""
    src = np.ascontiguousarray(src16, dtype=np.uint16)
    out = np.empty(src.shape, dtype=np.uint8)
    rc = load_library().ethcnn_narrow_rows_host(src.ctypes.data, out.ctypes.data, src.size, int(bit_depth))
    if rc:
        raise EthCnnError(rc, "narrow_rows_host: bit depth %d (8..16)" % bit_depth)
    return out


# ethcnn_compare_stats (200 bytes) and ethcnn_audit_result (216 bytes); the candidate is an ethcnn_sim_thr
COMPARE_THR = np.dtype([("up_k", "<i4", (3,)), ("down_k", "<i4", (3,))])
COMPARE_STATS = np.dtype([("ctus", "<u8"), ("rejected_ctus", "<u8"), ("over_tol", "<u8", (3,)), ("bits_diff", "<u8", (3,)), ("class_diff", "<u8", (3,)),
                          ("search_diff_ctus", "<u8"), ("checked_a", "<u8", (4,)), ("checked_b", "<u8", (4,)), ("worst_ctu", "<i8", (3,)),
                          ("max_abs", "<f4", (3,)), ("with_thr", "<u4")])
AUDIT_RESULT = np.dtype([("stats", COMPARE_STATS), ("plan", "<i4"), ("passes", "<i4"), ("fast_passes", "<i4"), ("reserved", "<i4")])
COMPARE_FLAG_REJECTED, COMPARE_FLAG_OVER_TOL, COMPARE_FLAG_CLASS, COMPARE_FLAG_SEARCH = 1, 2, 4, 8


def read_thr_info_k(path, order="ai"):
    """the six values of a Thr_info.txt on the k / 1024 grid (the nearest k each) -> (up_k [3], down_k [3]); order "ai": up1 down1 up2
    down2 up3 down3, "ldp": down1 up1 ...; ValueError for fewer than six numbers or a value outside the simulator's ranges"""
    tok = open(path).read().split()
    if len(tok) < 6:
        raise ValueError("%s: a Thr_info file holds six values" % path)
    k = [int(np.floor(float(t) * 1024 + 0.5)) for t in tok[:6]]
    a, b = k[0::2], k[1::2]
    up, down = (a, b) if order == "ai" else (b, a)
    if min(up) < 0 or max(up) > 1024 or min(down) < -1 or max(down) > 1024:
        raise ValueError("%s: thresholds outside [0, 1] (down: [-1/1024, 1])" % path)
    return up, down


def ctus_per_frame(width, height):
    return ((width + 63) // 64) * ((height + 63) // 64)


class DeviceBuffer(object):
    """HBM allocation owned by a context (ethcnn_device_alloc)."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = ctypes.c_void_p()
        ctx._chk(ctx.lib.ethcnn_device_alloc(ctx.h, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.lib.ethcnn_memcpy_h2d(self.ctx.h, self.ptr, arr.ctypes.data, arr.nbytes))

    def download(self, dtype, count):
        out = np.empty(int(count), dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.lib.ethcnn_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.lib.ethcnn_device_free(self.ctx.h, self.ptr)
            self.ptr = None


class EthCnn(object):
    """One predictor context on one GPU (the reference's tf.Session + Saver + graph)."""

    def __init__(self, device=0, max_ctus_per_pass=0, host_threads=0):
        self.lib = load_library()
        opt = Options(device=int(device), max_ctus_per_pass=int(max_ctus_per_pass), host_threads=int(host_threads))
        h = ctypes.c_void_p()
        rc = self.lib.ethcnn_create(ctypes.byref(h), ctypes.byref(opt))
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_last_error(None).decode())
        self.h = h

    # -- plumbing
    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            for t in list(getattr(self, "_trainers", ())):  # a trainer lives on this context: it goes first
                t.close()
            self.free_host_buffers()
            self.lib.ethcnn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def device_name(self):
        buf = ctypes.create_string_buffer(128)
        self._chk(self.lib.ethcnn_device_name(self.h, buf, 128))
        return buf.value.decode()

    @property
    def host_threads(self):
        """staging-fill threads of this context (the node budget divided by the local worker count)"""
        n = self.lib.ethcnn_host_threads(self.h)
        if n < 0:
            self._chk(n)
        return n

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def synchronize(self):
        self._chk(self.lib.ethcnn_synchronize(self.h))

    # -- weights / thresholds
    def load_checkpoint(self, prefix):
        self._chk(self.lib.ethcnn_load_checkpoint(self.h, os.fsencode(prefix)))

    def load_blob(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._chk(self.lib.ethcnn_load_blob(self.h, blob.ctypes.data_as(_fp), blob.size))

    def load_synthetic(self, seed=1, head_gain=1.0):
        self._chk(self.lib.ethcnn_load_synthetic(self.h, int(seed), float(head_gain)))

    def get_blob(self):
        out = np.empty(BLOB_FLOATS, dtype=np.float32)
        self._chk(self.lib.ethcnn_get_blob(self.h, out.ctypes.data_as(_fp), out.size))
        return out

    def load_thresholds(self, thr_info_path):
        self._chk(self.lib.ethcnn_load_thresholds(self.h, os.fsencode(thr_info_path)))

    def set_thresholds(self, thr_l1_lower, thr_l2_lower):
        self._chk(self.lib.ethcnn_set_thresholds(self.h, thr_l1_lower, thr_l2_lower))

    def get_thresholds(self):
        a, b = ctypes.c_float(), ctypes.c_float()
        self._chk(self.lib.ethcnn_get_thresholds(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # -- prediction
    def predict_luma(self, luma, width, height, nframes, qp, pitch=None, frame_stride=None):
        """Host luma planes (uint8 buffer) -> float32 [nframes*nctu, 21]."""
        luma = np.ascontiguousarray(luma, dtype=np.uint8)
        pitch = width if pitch is None else pitch
        frame_stride = pitch * height if frame_stride is None else frame_stride
        need = (nframes - 1) * frame_stride + (height - 1) * pitch + width if nframes else 0
        if luma.size < need:
            raise ValueError("luma buffer too small: %d < %d" % (luma.size, need))
        out = np.empty((nframes * ctus_per_frame(width, height), NOUT), dtype=np.float32)
        self._chk(self.lib.ethcnn_predict_luma(self.h, luma.ctypes.data, width, height, pitch, frame_stride,
                                               nframes, int(qp), out.ctypes.data_as(_fp)))
        return out

    def predict_luma_begin(self, luma_pinned, width, height, qp, probs_out):
        """streamed input (ethcnn_predict_luma_begin): queue ONE picture's pass on a host_buffer() the caller is still filling; report
        CTU rows with rows_ready (any thread), finish with predict_luma_end.  probs_out: float32 array of nctu * 21 (kept alive by
        the caller until predict_luma_end returns)"""
        n = ctus_per_frame(width, height)
        assert luma_pinned.dtype == np.uint8 and luma_pinned.flags["C_CONTIGUOUS"] and luma_pinned.size >= width * height
        assert probs_out.dtype == np.float32 and probs_out.size == n * NOUT and probs_out.flags["C_CONTIGUOUS"]
        self._chk(self.lib.ethcnn_predict_luma_begin(self.h, luma_pinned.ctypes.data, width, height, int(qp), probs_out.ctypes.data_as(_fp)))

    def predict_luma_end(self):
        self._chk(self.lib.ethcnn_predict_luma_end(self.h))

    def predict_luma_device(self, d_luma, width, height, nframes, qp, d_probs, pitch=None, frame_stride=None):
        """Both pointers already in HBM (ints or DeviceBuffer); asynchronous."""
        pitch = width if pitch is None else pitch
        frame_stride = pitch * height if frame_stride is None else frame_stride
        src = d_luma.ptr if isinstance(d_luma, DeviceBuffer) else int(d_luma)
        dst = d_probs.ptr if isinstance(d_probs, DeviceBuffer) else int(d_probs)
        self._chk(self.lib.ethcnn_predict_luma_device(self.h, src, width, height, pitch, frame_stride, nframes,
                                                      int(qp), dst))

    # -- high-bit-depth and non-4:2:0 sources
    def set_source_format(self, bit_depth=8, chroma=420):
        """what predict_yuv_file / _shard / _file_sharded / _range read from now on (default: 8-bit 4:2:0)"""
        fmt = SourceFormat(int(bit_depth), int(chroma))
        self._chk(self.lib.ethcnn_set_source_format(self.h, ctypes.addressof(fmt)))

    def source_format(self):
        fmt = SourceFormat()
        self._chk(self.lib.ethcnn_get_source_format(self.h, ctypes.addressof(fmt)))
        return fmt.bit_depth, fmt.chroma_format

    def set_narrow_chunk(self, frames=0):
        """frames per chunk of predict_luma16_device (0 = default: 256 MB of narrowed planes)"""
        self._chk(self.lib.ethcnn_set_narrow_chunk(self.h, int(frames)))

    def predict_luma16(self, luma16, width, height, nframes, qp, bit_depth, pitch_bytes=None, frame_stride_bytes=None):
        """Host luma planes of 16-bit samples (uint16 buffer) -> float32 [nframes*nctu, 21]: predict_luma on the narrowed planes."""
        luma16 = np.ascontiguousarray(luma16, dtype=np.uint16)
        pitch_bytes = 2 * width if pitch_bytes is None else pitch_bytes
        frame_stride_bytes = pitch_bytes * height if frame_stride_bytes is None else frame_stride_bytes
        need = (nframes - 1) * frame_stride_bytes + (height - 1) * pitch_bytes + 2 * width if nframes else 0
        if luma16.nbytes < need:
            raise ValueError("luma buffer too small: %d < %d bytes" % (luma16.nbytes, need))
        out = np.empty((nframes * ctus_per_frame(width, height), NOUT), dtype=np.float32)
        self._chk(self.lib.ethcnn_predict_luma16(self.h, luma16.ctypes.data, width, height, pitch_bytes, frame_stride_bytes, nframes,
                                                 int(bit_depth), int(qp), out.ctypes.data_as(_fp)))
        return out

    def predict_luma16_device(self, d_luma16, width, height, nframes, qp, bit_depth, d_probs, pitch_bytes=None, frame_stride_bytes=None):
        """Both pointers already in HBM (ints or DeviceBuffer); asynchronous."""
        pitch_bytes = 2 * width if pitch_bytes is None else pitch_bytes
        frame_stride_bytes = pitch_bytes * height if frame_stride_bytes is None else frame_stride_bytes
        src = d_luma16.ptr if isinstance(d_luma16, DeviceBuffer) else int(d_luma16)
        dst = d_probs.ptr if isinstance(d_probs, DeviceBuffer) else int(d_probs)
        self._chk(self.lib.ethcnn_predict_luma16_device(self.h, src, width, height, pitch_bytes, frame_stride_bytes, nframes,
                                                        int(bit_depth), int(qp), dst))

    def narrow_luma_device(self, d_src16, width, height, nframes, bit_depth, d_dst8, pitch_bytes=None, frame_stride_bytes=None,
                           dst_pitch=None, dst_frame_stride=None):
        """the narrowing kernel alone: 16-bit planes in HBM -> 8-bit planes of pitch roundup16(width) (pad columns zero); asynchronous"""
        pitch_bytes = 2 * width if pitch_bytes is None else pitch_bytes
        frame_stride_bytes = pitch_bytes * height if frame_stride_bytes is None else frame_stride_bytes
        dst_pitch = (width + 15) // 16 * 16 if dst_pitch is None else dst_pitch
        dst_frame_stride = dst_pitch * height if dst_frame_stride is None else dst_frame_stride
        src = d_src16.ptr if isinstance(d_src16, DeviceBuffer) else int(d_src16)
        dst = d_dst8.ptr if isinstance(d_dst8, DeviceBuffer) else int(d_dst8)
        self._chk(self.lib.ethcnn_narrow_luma_device(self.h, src, width, height, pitch_bytes, frame_stride_bytes, nframes, int(bit_depth),
                                                     dst, dst_pitch, dst_frame_stride))

    def predict_ctus(self, ctus, qp):
        """[n,64,64] uint8 CTUs -> [n,21]; gates per <=1024-CTU sub-batch exactly like
        get_y_conv_on_large_data (video_to_cu_depth.py:61-73): a 64-wide, 64n-tall 'frame'."""
        ctus = np.ascontiguousarray(ctus, dtype=np.uint8).reshape(-1, 64, 64)
        n = ctus.shape[0]
        if n == 0:
            return np.zeros((0, NOUT), dtype=np.float32)
        return self.predict_luma(ctus.reshape(-1), 64, 64 * n, 1, qp)

    def predict_yuv_file(self, yuv_path, width, height, qp, out_path):
        nf = ctypes.c_int64(0)
        self._chk(self.lib.ethcnn_predict_yuv_file(self.h, os.fsencode(yuv_path), width, height, int(qp),
                                                   os.fsencode(out_path), ctypes.byref(nf)))
        return nf.value

    def predict_yuv_file_sharded(self, devices, yuv_path, width, height, qp, out_path):
        """the whole file over `devices` (HIP ordinals; devices[0] = this context's) from this process: a worker thread per entry
        (ethcnn_predict_yuv_file_sharded; ctypes releases the GIL for the call)"""
        nf = ctypes.c_int64(0)
        arr = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
        self._chk(self.lib.ethcnn_predict_yuv_file_sharded(self.h, arr, len(devices), os.fsencode(yuv_path), width, height, int(qp),
                                                           os.fsencode(out_path), ctypes.byref(nf)))
        return nf.value

    def startup_times(self):
        """(ms of ethcnn_create's first HIP call = runtime initialisation, ms of the whole ethcnn_create)"""
        a, b = ctypes.c_double(), ctypes.c_double()
        self._chk(self.lib.ethcnn_get_startup_times(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def predict_yuv_range(self, yuv_path, width, height, qp, out_path, frame_begin, frame_end):
        """frames [frame_begin, frame_end) -> an out_path holding exactly those (get_prob's n_frames_start / n_frames_end)"""
        self._chk(self.lib.ethcnn_predict_yuv_range(self.h, os.fsencode(yuv_path), width, height, int(qp),
                                                    os.fsencode(out_path), int(frame_begin), int(frame_end)))
        return int(frame_end) - int(frame_begin)

    def predict_yuv_shard(self, yuv_path, width, height, qp, out_path, frame_begin, frame_end):
        self._chk(self.lib.ethcnn_predict_yuv_shard(self.h, os.fsencode(yuv_path), width, height, int(qp),
                                                    os.fsencode(out_path), int(frame_begin), int(frame_end)))

    def resi_vectors(self, luma, width, height, pitch=None):
        luma = np.ascontiguousarray(luma, dtype=np.uint8)
        pitch = width if pitch is None else pitch
        need = (height - 1) * pitch + width if width > 0 and height > 0 else 0
        if luma.size < need:
            raise ValueError("luma buffer too small: %d < %d" % (luma.size, need))
        out = np.empty((ctus_per_frame(width, height), NVEC), dtype=np.float32)
        self._chk(self.lib.ethcnn_resi_vectors(self.h, luma.ctypes.data, width, height, pitch, out.ctypes.data_as(_fp)))
        return out

    def resi_vectors_device(self, d_luma, width, height, d_vec, pitch=None):
        """asynchronous: LDP front-end on device buffers (ethcnn_resi_vectors_device)"""
        pitch = width if pitch is None else pitch
        self._chk(self.lib.ethcnn_resi_vectors_device(self.h, d_luma.ptr, width, height, pitch, d_vec.ptr))

    # -- config #5 back-end: ETH-LSTM one step (resi_to_cu_depth_LDP.py:108-129)
    def load_lstm_checkpoint(self, prefix):
        self._chk(self.lib.ethcnn_load_lstm_checkpoint(self.h, os.fsencode(prefix)))

    def load_lstm_blob(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._chk(self.lib.ethcnn_load_lstm_blob(self.h, blob.ctypes.data_as(_fp), blob.size))

    def load_lstm_synthetic(self, seed=1, head_gain=1.0):
        self._chk(self.lib.ethcnn_load_lstm_synthetic(self.h, int(seed), float(head_gain)))

    def get_lstm_blob(self):
        out = np.empty(LSTM_BLOB_FLOATS, dtype=np.float32)
        self._chk(self.lib.ethcnn_get_lstm_blob(self.h, out.ctypes.data_as(_fp), out.size))
        return out

    def lstm_step(self, vec, state_in, qp, i_frame):
        """vec [n,448], state_in [n,2,448] or None -> (probs [n,21] gated, state_out [n,2,448]); the
        vectors go through HBM buffers and the *_device entry point."""
        vec = np.ascontiguousarray(vec, dtype=np.float32)
        n = vec.shape[0]
        dv, dso, dp = self.alloc(vec.nbytes), self.alloc(n * 2 * NVEC * 4), self.alloc(n * NOUT * 4)
        dv.upload(vec)
        dsi = None
        if state_in is not None:
            state_in = np.ascontiguousarray(state_in, dtype=np.float32).reshape(n, 2, NVEC)
            dsi = self.alloc(state_in.nbytes)
            dsi.upload(state_in)
        self._chk(self.lib.ethcnn_lstm_step_device(self.h, dv.ptr, dsi.ptr if dsi else None, n, int(qp), int(i_frame),
                                                   dso.ptr, dp.ptr))
        probs = dp.download(np.float32, n * NOUT).reshape(n, NOUT)
        state = dso.download(np.float32, n * 2 * NVEC).reshape(n, 2, NVEC)
        for b in (dv, dso, dp, dsi):
            if b is not None:
                b.free()
        return probs, state

    def ldp_predict_frame(self, luma, width, height, qp, i_frame, state_in=None, pitch=None):
        """one frame of resi.yuv luma -> (probs [nctu,21], state_out [nctu,2,448])"""
        luma = np.ascontiguousarray(luma, dtype=np.uint8)
        pitch = width if pitch is None else pitch
        need = (height - 1) * pitch + width if width > 0 and height > 0 else 0
        if luma.size < need:
            raise ValueError("luma buffer too small: %d < %d" % (luma.size, need))
        n = ctus_per_frame(width, height)
        probs = np.empty((n, NOUT), dtype=np.float32)
        state = np.empty((n, 2, NVEC), dtype=np.float32)
        sin = None
        if state_in is not None:
            sin = np.ascontiguousarray(state_in, dtype=np.float32).reshape(n, 2, NVEC)
        self._chk(self.lib.ethcnn_ldp_predict_frame(self.h, luma.ctypes.data, width, height, pitch, int(qp), int(i_frame),
                                                    sin.ctypes.data if sin is not None else None,
                                                    state.ctypes.data_as(_fp), probs.ctypes.data_as(_fp)))
        return probs, state

    def ldp_step(self, luma, width, height, qp, i_frame, state_in=None, pitch=None, probs_out=None):
        """one frame with the recurrent state resident in HBM between calls (ethcnn_ldp_step): state_in None = the
        previous call's state (zeros when i_frame <= 1) -> probs [nctu, 21]"""
        luma = np.ascontiguousarray(luma, dtype=np.uint8)
        pitch = width if pitch is None else pitch
        need = (height - 1) * pitch + width if width > 0 and height > 0 else 0
        if luma.size < need:
            raise ValueError("luma buffer too small: %d < %d" % (luma.size, need))
        n = ctus_per_frame(width, height)
        probs = np.empty((n, NOUT), dtype=np.float32) if probs_out is None else probs_out
        assert probs.dtype == np.float32 and probs.size == n * NOUT and probs.flags["C_CONTIGUOUS"]
        sin = None
        if state_in is not None:
            sin = np.ascontiguousarray(state_in, dtype=np.float32).reshape(n, 2, NVEC)
        self._chk(self.lib.ethcnn_ldp_step(self.h, luma.ctypes.data, width, height, pitch, int(qp), int(i_frame),
                                           sin.ctypes.data if sin is not None else None, probs.ctypes.data_as(_fp)))
        return probs.reshape(n, NOUT)

    def ldp_step_begin(self, luma_pinned, width, height, qp, i_frame, probs_out, state_in=None, pitch=None):
        """streamed input (ethcnn_ldp_step_begin): queue the frame's kernels on a host_buffer() the caller is still filling; report
        rows with rows_ready (any thread), finish with ldp_step_end.  probs_out: float32 array of nctu * 21 (kept alive by the
        caller until ldp_step_end returns)"""
        pitch = width if pitch is None else pitch
        n = ctus_per_frame(width, height)
        assert luma_pinned.dtype == np.uint8 and luma_pinned.flags["C_CONTIGUOUS"] and luma_pinned.size >= (height - 1) * pitch + width
        assert probs_out.dtype == np.float32 and probs_out.size == n * NOUT and probs_out.flags["C_CONTIGUOUS"]
        sin = None
        if state_in is not None:
            sin = np.ascontiguousarray(state_in, dtype=np.float32).reshape(n, 2, NVEC)
        self._chk(self.lib.ethcnn_ldp_step_begin(self.h, luma_pinned.ctypes.data, width, height, pitch, int(qp), int(i_frame),
                                                 sin.ctypes.data if sin is not None else None, probs_out.ctypes.data_as(_fp)))

    def rows_ready(self, ctu_row_begin, ctu_row_end):
        if self.lib.ethcnn_rows_ready(self.h, int(ctu_row_begin), int(ctu_row_end)) != 0:
            raise ValueError("rows_ready(%d, %d)" % (ctu_row_begin, ctu_row_end))

    def ldp_step_end(self):
        self._chk(self.lib.ethcnn_ldp_step_end(self.h))

    def ldp_get_state(self, width, height):
        n = ctus_per_frame(width, height)
        state = np.empty((n, 2, NVEC), dtype=np.float32)
        self._chk(self.lib.ethcnn_ldp_get_state(self.h, state.ctypes.data_as(_fp), state.size))
        return state

    # -- config #5 offline: a whole residual sequence = the per-frame ldp_step loop, bit for bit, scheduled for throughput
    def ldp_sequence(self, luma, width, height, nframes, qp, i_frame_first=1, state_in=None, pitch=None, frame_stride=None,
                     probs_out=None):
        """luma: uint8 frames in host memory (pageable or a host_buffer()) -> probs [nframes, nctu, 21]; frame t carries
        i_frame_first + t; state_in None = zeros (i_frame <= 1) or the resident state.  The final state stays resident
        (ldp_get_state, or continue with ldp_step)."""
        assert luma.dtype == np.uint8 and luma.flags["C_CONTIGUOUS"]
        pitch = width if pitch is None else pitch
        frame_stride = pitch * height if frame_stride is None else frame_stride
        need = (nframes - 1) * frame_stride + (height - 1) * pitch + width if min(width, height, nframes) > 0 else 0
        if luma.size < need:
            raise ValueError("luma buffer too small: %d < %d" % (luma.size, need))
        n = ctus_per_frame(width, height)
        probs = np.empty((max(nframes, 0), n, NOUT), dtype=np.float32) if probs_out is None else probs_out
        assert probs.dtype == np.float32 and probs.size == max(nframes, 0) * n * NOUT and probs.flags["C_CONTIGUOUS"]
        sin = None
        if state_in is not None:
            sin = np.ascontiguousarray(state_in, dtype=np.float32).reshape(n, 2, NVEC)
        self._chk(self.lib.ethcnn_ldp_sequence(self.h, luma.ctypes.data, width, height, pitch, frame_stride, int(nframes), int(qp),
                                               int(i_frame_first), sin.ctypes.data if sin is not None else None,
                                               probs.ctypes.data_as(_fp)))
        return probs.reshape(max(nframes, 0), n, NOUT)

    def ldp_sequence_device(self, d_luma, width, height, nframes, qp, i_frame_first, d_probs, d_state_in=None, pitch=None,
                            frame_stride=None):
        """asynchronous on the context's stream (ethcnn_ldp_sequence_device): device buffers (alloc()) or raw device addresses"""
        pitch = width if pitch is None else pitch
        frame_stride = pitch * height if frame_stride is None else frame_stride
        ptr = lambda b: None if b is None else getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_ldp_sequence_device(self.h, ptr(d_luma), width, height, pitch, frame_stride, int(nframes), int(qp),
                                                      int(i_frame_first), ptr(d_state_in), ptr(d_probs)))

    def ldp_predict_yuv_file(self, resi_yuv_path, width, height, qp, out_path, frame_begin, frame_end):
        """frames [frame_begin, frame_end) of a 4:2:0 residual file (frame k = POC k, frame_begin >= 1) -> out_path, float32
        [frames][nctu][21]"""
        self._chk(self.lib.ethcnn_ldp_predict_yuv_file(self.h, os.fsencode(resi_yuv_path), width, height, int(qp),
                                                       os.fsencode(out_path), int(frame_begin), int(frame_end)))
        return int(frame_end) - int(frame_begin)

    def ldp_set_sequence_chunk(self, frames):
        self._chk(self.lib.ethcnn_ldp_set_sequence_chunk(self.h, int(frames)))

    def host_buffer(self, nbytes):
        """pinned host memory as a uint8 numpy array (freed with the context, or by free_host_buffer)"""
        p = _vp()
        self._chk(self.lib.ethcnn_host_alloc(self.h, int(nbytes), ctypes.byref(p)))
        arr = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(max(1, int(nbytes)),))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p.value)
        return arr[:nbytes]

    def free_host_buffer(self, arr):
        """frees one host_buffer() (the array it returned, or a view that starts at its first byte)"""
        ptr = arr.ctypes.data
        if ptr not in getattr(self, "_pinned", []):
            raise ValueError("not a host_buffer() of this context")
        self.lib.ethcnn_host_free(self.h, ptr)
        self._pinned.remove(ptr)

    def free_host_buffers(self):
        for ptr in getattr(self, "_pinned", []):
            self.lib.ethcnn_host_free(self.h, ptr)
        self._pinned = []

    # -- measurement / introspection
    def set_profiling(self, level=2):
        """0 off, 1 dominant kernel (FC1) only, 2 every stage."""
        self._chk(self.lib.ethcnn_set_profiling(self.h, int(level)))

    def set_pass_pipeline(self, on=True):
        """CTU-load stage of pass i+1 beside FC1 of pass i (default on); off = one stream, stage timings do not overlap"""
        self._chk(self.lib.ethcnn_set_pass_pipeline(self.h, 1 if on else 0))

    def measure_mfma_rate(self, seconds=0.05):
        """TFLOP/s of pure exact-fp32 MFMAs this GPU sustains (box calibration for reading roofline fractions)"""
        v = ctypes.c_double(0.0)
        self._chk(self.lib.ethcnn_measure_mfma_rate(self.h, float(seconds), ctypes.byref(v)))
        return v.value

    def set_fc1_plan(self, plan=3):
        """arithmetic plan of big passes: 0 = exact fp32 (default, bit-identical to the oracle); 2 = FC1 as two-way fp16 splits on the
        16-bit matrix pipe; 3 = trunk, FC1 and heads that way (as accurate against float64, NOT bit-identical; include/ethcnn.h)."""
        self._chk(self.lib.ethcnn_set_fc1_plan(self.h, int(plan)))

    def fc1_plan(self):
        return int(self.lib.ethcnn_get_fc1_plan(self.h))

    def check_fc1_plan(self, plan):
        """the load-time accuracy guard of plans 2 / 3 for the loaded weights (ethcnn_check_fc1_plan) ->
        {"accepted", "apriori_bound", "measured" (None: the a-priori bound sufficed), "message"}; never raises for a refusal"""
        b, m = ctypes.c_double(0.0), ctypes.c_double(-1.0)
        rc = self.lib.ethcnn_check_fc1_plan(self.h, int(plan), ctypes.byref(b), ctypes.byref(m))
        if rc not in (0, ERR_PLAN_REFUSED):
            self._chk(rc)
        return {"accepted": rc == 0, "apriori_bound": b.value, "measured": None if m.value < 0 else m.value,
                "message": "" if rc == 0 else self.lib.ethcnn_last_error(self.h).decode()}

    # -- comparing two predictions, auditing a plan (include/ethcnn.h "comparing two predictions")
    @staticmethod
    def _compare_thr(thr):
        """None, or one candidate as a SIM_THR record / (up_k, down_k) -> (keep-alive array or None, pointer or None)"""
        if thr is None:
            return None, None
        t = np.zeros(1, COMPARE_THR)
        if isinstance(thr, np.ndarray) and thr.dtype == COMPARE_THR:
            t[0] = thr.reshape(-1)[0]
        else:
            t["up_k"][0], t["down_k"][0] = thr[0], thr[1]
        return t, t.ctypes.data

    @staticmethod
    def _stats_dict(rec):
        out = {}
        for name in rec.dtype.names:
            v = rec[name]
            if isinstance(v, np.void):
                out.update(EthCnn._stats_dict(v))
            elif name != "reserved":
                out[name] = v.tolist() if isinstance(v, np.ndarray) else v.item()
        return out

    @staticmethod
    def _pair(a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype != np.float32 or b.dtype != np.float32 or not a.flags["C_CONTIGUOUS"] or not b.flags["C_CONTIGUOUS"]:
            a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        if a.size != b.size or a.size % NOUT:
            raise ValueError("two arrays of the same number of CTUs x 21 are required")
        return a, b

    def _compare_host(self, a, b, width, height, nframes, tol, thr, want_flags):
        a, b = self._pair(a, b)
        n = a.size // NOUT
        keep, tp = self._compare_thr(thr)
        st = np.zeros(1, COMPARE_STATS)
        flags = None
        if want_flags is not False and want_flags is not None:
            flags = want_flags if isinstance(want_flags, np.ndarray) else np.zeros(n, np.uint8)
            assert flags.dtype == np.uint8 and flags.size == n and flags.flags["C_CONTIGUOUS"]
        fp = flags.ctypes.data if flags is not None and n else None
        if width is None:
            rc = self.lib.ethcnn_compare_probs(self.h, a.ctypes.data, b.ctypes.data, n, float(tol), tp, st.ctypes.data, fp)
        else:
            per = ctus_per_frame(width, height)
            nframes = n // per if nframes is None else int(nframes)
            if nframes * per != n:
                raise ValueError("%d CTUs are not %d frames of %d x %d" % (n, nframes, width, height))
            rc = self.lib.ethcnn_compare_frames(self.h, a.ctypes.data, b.ctypes.data, int(width), int(height), nframes, float(tol), tp, st.ctypes.data, fp)
        self._chk(rc)
        out = self._stats_dict(st[0])
        if flags is not None:
            out["flags"] = flags
        return out

    def compare_probs(self, a, b, tol, thr=None, want_flags=False):
        """two host arrays float32 [n, 21] (per-CTU layout) -> dict of the fields of ethcnn_compare_stats (+ "flags" uint8 [n] with
        want_flags: True, or a uint8 array to fill, which may lie in a host_buffer())"""
        return self._compare_host(a, b, None, None, None, tol, thr, want_flags)

    def compare_frames(self, a, b, width, height, tol, thr=None, want_flags=False, nframes=None):
        """the frame layout: whole frames of width x height (multiples of 8)"""
        return self._compare_host(a, b, width, height, nframes, tol, thr, want_flags)

    def compare_probs_device(self, d_a, d_b, n, tol, thr=None, d_flags=None):
        """pointers in HBM (ints or DeviceBuffer), 4-byte aligned; synchronous"""
        keep, tp = self._compare_thr(thr)
        st = np.zeros(1, COMPARE_STATS)
        ptr = lambda x: None if x is None else x.ptr if isinstance(x, DeviceBuffer) else int(x)
        self._chk(self.lib.ethcnn_compare_probs_device(self.h, ptr(d_a), ptr(d_b), int(n), float(tol), tp, st.ctypes.data, ptr(d_flags)))
        return self._stats_dict(st[0])

    def compare_frames_device(self, d_a, d_b, width, height, nframes, tol, thr=None, d_flags=None):
        keep, tp = self._compare_thr(thr)
        st = np.zeros(1, COMPARE_STATS)
        ptr = lambda x: None if x is None else x.ptr if isinstance(x, DeviceBuffer) else int(x)
        self._chk(self.lib.ethcnn_compare_frames_device(self.h, ptr(d_a), ptr(d_b), int(width), int(height), int(nframes), float(tol), tp,
                                                        st.ctypes.data, ptr(d_flags)))
        return self._stats_dict(st[0])

    def audit_plan_bytes(self, width, height, nframes):
        return int(self.lib.ethcnn_audit_plan_bytes(int(width), int(height), int(nframes)))

    def audit_plan(self, lumas, width, height, nframes, qp, plan, tol=1e-4, thr=None, pitch=None, frame_stride=None):
        """plan 2 / 3 against the exact plan over the caller's frames, open gates (ethcnn_audit_plan_device) -> dict of the fields of
        ethcnn_audit_result.  lumas: a device pointer (int or DeviceBuffer), or a host uint8 array that is uploaded for the call."""
        pitch = width if pitch is None else pitch
        frame_stride = pitch * height if frame_stride is None else frame_stride
        keep, tp = self._compare_thr(thr)
        res = np.zeros(1, AUDIT_RESULT)
        own = None
        if isinstance(lumas, DeviceBuffer):
            src = lumas.ptr
        elif isinstance(lumas, (int, np.integer)):
            src = int(lumas)
        else:
            lumas = np.ascontiguousarray(lumas, dtype=np.uint8)
            need = (nframes - 1) * frame_stride + (height - 1) * pitch + width if nframes else 0
            if lumas.size < need:
                raise ValueError("luma buffer too small: %d < %d" % (lumas.size, need))
            own = self.alloc(max(1, lumas.nbytes))
            own.upload(lumas)
            src = own.ptr
        try:
            self._chk(self.lib.ethcnn_audit_plan_device(self.h, src, int(width), int(height), pitch, frame_stride, int(nframes), int(qp), int(plan),
                                                        float(tol), tp, res.ctypes.data))
        finally:
            if own is not None:
                own.free()
        return self._stats_dict(res[0])

    def audit_plan_yuv_file(self, yuv_path, width, height, qp, plan, first=0, step=1, count=1, tol=1e-4, thr=None):
        """frames first + i * step, i < count, of an 8-bit 4:2:0 file (ethcnn_audit_plan_yuv_file)"""
        keep, tp = self._compare_thr(thr)
        res = np.zeros(1, AUDIT_RESULT)
        self._chk(self.lib.ethcnn_audit_plan_yuv_file(self.h, os.fsencode(yuv_path), int(width), int(height), int(qp), int(plan), int(first), int(step),
                                                      int(count), float(tol), tp, res.ctypes.data))
        return self._stats_dict(res[0])

    def set_small_pass_launch(self, on=True):
        """one picture (<= 2304 CTUs, 16-byte aligned rows) as ONE launch (default on); off = five launches.  Same results."""
        self._chk(self.lib.ethcnn_set_small_pass_launch(self.h, 1 if on else 0))

    def reset_stage_times(self):
        self._chk(self.lib.ethcnn_reset_stage_times(self.h))

    def stage_times(self):
        st = StageTimes()
        self._chk(self.lib.ethcnn_get_stage_times(self.h, ctypes.byref(st)))
        return {"ms": dict(zip(STAGES, list(st.ms))), "launches": dict(zip(STAGES, list(st.launches))), "ctus": st.ctus,
                "timed": dict(zip(STAGES, list(st.timed))), "timed_ctus": dict(zip(STAGES, list(st.timed_ctus))),
                "timing_errors": st.timing_errors}

    def set_debug_capture(self, on=True):
        """store FC2 outputs, logits and ungated probabilities of the following passes (debug_fetch)"""
        self._chk(self.lib.ethcnn_set_debug_capture(self.h, 1 if on else 0))

    def debug_fetch(self, which, n):
        out = np.empty((n, _DBG_WIDTH[which]), dtype=np.float32)
        self._chk(self.lib.ethcnn_debug_fetch(self.h, which, out.ctypes.data_as(_fp), out.size))
        return out


# ---------------------------------------------------------------------------------------------------------------- training ---
TRAIN_REC = 4992  # bytes per training-sample record (4096 luma, 64 pad, 52 x 16 label bytes)
LDP_REC = 16516   # bytes per LDP record: 64 header bytes, then 4 slots of [QP byte | 16 label bytes | 4096 residual bytes]
LDP_SLOT_BASE, LDP_SLOT_BYTES = 64, 4113
SET_TRAIN, SET_VALID = 0, 1
TRAIN_NET_AI, TRAIN_NET_LDP = 0, 1
TDBG_GRADS, TDBG_MASK_FC1, TDBG_MASK_FC2, TDBG_PROBS, TDBG_INDICES, TDBG_ACCUM, TDBG_H1 = range(7)
_M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def mixed_eval_slots(seed, n):
    """slot (0..3) of sample i = 0 .. n-1 in an LDP evaluation at qp = -1: (draw(2, 0, i, 0) >> 32) * 4 >> 32 (include/ethcnn.h)"""
    base = _mix64(_mix64((int(seed) ^ 2 * 0xD1B54A32D192ED03) & _M64) ^ 0)  # draw(2, step 0, ...) up to its last mix
    return np.array([(_mix64(base ^ (i << 12)) >> 32) * 4 >> 32 for i in range(int(n))], dtype=np.int64)


class TrainOptions(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int), ("lr_init", ctypes.c_float), ("momentum", ctypes.c_float), ("decay_rate", ctypes.c_float),
                ("decay_steps", ctypes.c_int64), ("dropout", ctypes.c_int), ("seed", ctypes.c_uint64), ("net", ctypes.c_int),
                ("tune", ctypes.c_int), ("reserved", ctypes.c_int * 6)]


class Trainer(object):
    """ETH-CNN training on the GPU of an EthCnn context (include/ethcnn.h "training").  Defaults are the reference's
    (train_CNN_CTU64.py:36-47): batch 64, lr 0.01 decayed by 0.3163 every 250000 steps, momentum 0.9, dropout on.
    net="ai": the All-Intra net on 4992-byte records; net="ldp": the Low-Delay-P residual net on 16516-byte records
    (train_resi_CNN_CTU64.py).  tune: PARTLY_TUNING_MODE, 0 = every tensor, 1 / 2 / 3 = only head 64 / 32 / 16."""

    def __init__(self, ctx, batch=64, lr=0.01, momentum=0.9, decay_rate=0.3163, decay_steps=250000, dropout=True, seed=0, net="ai",
                 tune=0):
        self.ctx, self.lib, self.batch, self.seed = ctx, ctx.lib, int(batch), int(seed) & (2 ** 64 - 1)
        nets = {"ai": TRAIN_NET_AI, "ldp": TRAIN_NET_LDP}
        self.net = net
        o = TrainOptions(int(batch), float(lr), float(momentum), float(decay_rate), int(decay_steps), 1 if dropout else 0,
                         int(seed) & (2 ** 64 - 1), nets[net] if net in nets else int(net), int(tune))
        h = ctypes.c_void_p()
        rc = self.lib.ethcnn_train_create(ctx.h, ctypes.byref(o), ctypes.byref(h))
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_last_error(ctx.h).decode())
        self.h = h
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)

    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_train_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_train_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def init_weights(self, seed):
        self._chk(self.lib.ethcnn_train_init_weights(self.h, int(seed) & (2 ** 64 - 1)))

    def set_blob(self, blob, accum=None):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        acc = None if accum is None else np.ascontiguousarray(accum, dtype=np.float32)
        if acc is not None and acc.size != blob.size:
            raise ValueError("accumulators and blob differ in size")
        self._chk(self.lib.ethcnn_train_set_blob(self.h, blob.ctypes.data_as(_fp), None if acc is None else acc.ctypes.data_as(_fp),
                                                 blob.size))

    def get_blob(self, with_accum=False):
        blob = np.empty(BLOB_FLOATS, dtype=np.float32)
        acc = np.empty(BLOB_FLOATS, dtype=np.float32) if with_accum else None
        self._chk(self.lib.ethcnn_train_get_blob(self.h, blob.ctypes.data_as(_fp), None if acc is None else acc.ctypes.data_as(_fp),
                                                 BLOB_FLOATS))
        return (blob, acc) if with_accum else blob

    def set_samples(self, which, records, take=False):
        """records: bytes / uint8 array of whole 4992-byte records (LDP: 16516-byte records), one sample file of the reference's
        Extract_Data; or a built SampleSet, which stays in HBM (take=True: the trainer adopts its buffer and the set becomes empty,
        else a device-to-device copy)"""
        if isinstance(records, SampleSet):
            self._chk(self.lib.ethcnn_train_set_samples_from(self.h, int(which), records.h, 1 if take else 0))
            return
        buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records, np.uint8)
        self._chk(self.lib.ethcnn_train_set_samples(self.h, int(which), buf.ctypes.data if buf.size else None, buf.size))

    def set_qps(self, qps):
        arr = (ctypes.c_int * len(qps))(*[int(q) for q in qps])
        self._chk(self.lib.ethcnn_train_set_qps(self.h, arr, len(qps)))

    def run(self, first_step, nsteps):
        """enqueue steps first_step .. first_step + nsteps - 1 (device-drawn batches); returns at once"""
        self._chk(self.lib.ethcnn_train_run(self.h, int(first_step), int(nsteps)))

    def last_stats(self):
        """(loss_list, accuracy_list) of the last step enqueued (waits for it)"""
        l3, a3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._chk(self.lib.ethcnn_train_last_stats(self.h, l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp)))
        return l3, a3

    def step_indices(self, step, idx, qps):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        qps = np.ascontiguousarray(np.broadcast_to(np.asarray(qps, dtype=np.int32), idx.shape))
        l3, a3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._chk(self.lib.ethcnn_train_step_indices(self.h, int(step), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                     qps.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), idx.size,
                                                     l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp)))
        return l3, a3

    def evaluate(self, which, qp, idx=None, n=None, want_probs=False):
        """(loss_list, accuracy_list[, probs [n,21]]) of ONE forward batch over the samples idx (or 0 .. n-1); LDP: qp = -1 puts
        sample i at slot mixed_eval_slots(seed, n)[i]"""
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            n = idx.size
        probs = np.empty((int(n), NOUT), dtype=np.float32) if want_probs else None
        l3, a3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._chk(self.lib.ethcnn_train_evaluate(self.h, int(which), None if idx is None else idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                 int(n), int(qp), l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp),
                                                 None if probs is None else probs.ctypes.data_as(_fp)))
        return (l3, a3, probs) if want_probs else (l3, a3)

    def debug_fetch(self, which):
        n = {TDBG_GRADS: BLOB_FLOATS, TDBG_ACCUM: BLOB_FLOATS, TDBG_MASK_FC1: self.batch * NVEC, TDBG_MASK_FC2: self.batch * NFC2,
             TDBG_PROBS: self.batch * NOUT, TDBG_INDICES: self.batch * 2, TDBG_H1: self.batch * NVEC}[which]
        out = np.empty(n, dtype=np.float32)
        self._chk(self.lib.ethcnn_train_debug_fetch(self.h, int(which), out.ctypes.data_as(_fp), n))
        return out


def _train_options_array(opts):
    opts = list(opts)
    for o in opts:
        if not isinstance(o, TrainOptions):
            raise TypeError("a trainer group takes TrainOptions, got %r" % type(o).__name__)
    return (TrainOptions * max(len(opts), 1))(*opts), len(opts)


def train_options(batch=64, lr=0.01, momentum=0.9, decay_rate=0.3163, decay_steps=250000, dropout=True, seed=0, net="ai", tune=0):
    """the TrainOptions of Trainer's keyword arguments (a TrainerGroup takes a list of them)"""
    nets = {"ai": TRAIN_NET_AI, "ldp": TRAIN_NET_LDP}
    return TrainOptions(int(batch), float(lr), float(momentum), float(decay_rate), int(decay_steps), 1 if dropout else 0,
                        int(seed) & _M64, nets[net] if net in nets else int(net), int(tune))


def train_group_check(opts, lib=None):
    """host-only check of a trainer group's options (no context): raises EthCnnError(ERR_ARG) naming the member and the field"""
    lib = lib or load_library()
    arr, k = _train_options_array(opts)
    err = ctypes.create_string_buffer(256)
    rc = lib.ethcnn_train_group_check(arr, k, err, len(err))
    if rc:
        raise EthCnnError(rc, err.value.decode())


class TrainerGroup(object):
    """K (1..8) independent ETH-CNN trainers in every launch of a step (include/ethcnn.h "training, several models at once"):
    one context, one stream, one copy of the sample sets.  Member m computes what Trainer computes with opts[m], bit for bit.
    opts: a list of TrainOptions (train_options(...)) with the same net, batch and tune."""

    def __init__(self, ctx, opts):
        self.ctx, self.lib = ctx, ctx.lib
        arr, k = _train_options_array(opts)
        h = ctypes.c_void_p()
        rc = self.lib.ethcnn_train_group_create(ctx.h, arr, k, ctypes.byref(h))
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_last_error(ctx.h).decode())
        self.h, self.k, self.batch = h, k, int(arr[0].batch)
        self.seeds = [int(arr[m].seed) for m in range(k)]
        self.net = "ldp" if arr[0].net == TRAIN_NET_LDP else "ai"
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)

    def __len__(self):
        return self.k

    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_train_group_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_train_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def init_weights(self, seeds):
        """seeds: one per member, or one number for all"""
        seeds = [seeds] * self.k if np.isscalar(seeds) else list(seeds)
        if len(seeds) != self.k:
            raise ValueError("%d seeds for %d members" % (len(seeds), self.k))
        self._chk(self.lib.ethcnn_train_group_init_weights(self.h, (ctypes.c_uint64 * self.k)(*[int(x) & _M64 for x in seeds])))

    def set_blob(self, m, blob, accum=None):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        acc = None if accum is None else np.ascontiguousarray(accum, dtype=np.float32)
        if acc is not None and acc.size != blob.size:
            raise ValueError("accumulators and blob differ in size")
        self._chk(self.lib.ethcnn_train_group_set_blob(self.h, int(m), blob.ctypes.data_as(_fp),
                                                       None if acc is None else acc.ctypes.data_as(_fp), blob.size))

    def get_blob(self, m, with_accum=False):
        blob = np.empty(BLOB_FLOATS, dtype=np.float32)
        acc = np.empty(BLOB_FLOATS, dtype=np.float32) if with_accum else None
        self._chk(self.lib.ethcnn_train_group_get_blob(self.h, int(m), blob.ctypes.data_as(_fp),
                                                       None if acc is None else acc.ctypes.data_as(_fp), BLOB_FLOATS))
        return (blob, acc) if with_accum else blob

    def set_samples(self, which, records, take=False):
        """what Trainer.set_samples takes; one copy in HBM serves every member"""
        if isinstance(records, SampleSet):
            self._chk(self.lib.ethcnn_train_group_set_samples_from(self.h, int(which), records.h, 1 if take else 0))
            return
        buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records, np.uint8)
        self._chk(self.lib.ethcnn_train_group_set_samples(self.h, int(which), buf.ctypes.data if buf.size else None, buf.size))

    def set_qps(self, m, qps):
        arr = (ctypes.c_int * len(qps))(*[int(q) for q in qps])
        self._chk(self.lib.ethcnn_train_group_set_qps(self.h, int(m), arr, len(qps)))

    def run(self, first_step, nsteps):
        """enqueue steps first_step .. first_step + nsteps - 1 of every member (device-drawn batches); returns at once"""
        self._chk(self.lib.ethcnn_train_group_run(self.h, int(first_step), int(nsteps)))

    def last_stats(self):
        """(loss_list [k,3], accuracy_list [k,3]) of the last step enqueued (waits for it)"""
        l3, a3 = np.zeros((self.k, 3), np.float32), np.zeros((self.k, 3), np.float32)
        self._chk(self.lib.ethcnn_train_group_last_stats(self.h, l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp)))
        return l3, a3

    def step_indices(self, step, idx, qps):
        """idx [k, batch]; qps [k, batch], or anything that broadcasts to it"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.shape != (self.k, self.batch):
            raise ValueError("idx must be [%d, %d]" % (self.k, self.batch))
        qps = np.ascontiguousarray(np.broadcast_to(np.asarray(qps, dtype=np.int32), idx.shape))
        l3, a3 = np.zeros((self.k, 3), np.float32), np.zeros((self.k, 3), np.float32)
        self._chk(self.lib.ethcnn_train_group_step_indices(self.h, int(step), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                           qps.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), self.batch,
                                                           l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp)))
        return l3, a3

    def evaluate(self, which, qps, idx=None, n=None, want_probs=False):
        """(loss_list [k,3], accuracy_list [k,3][, probs [k,n,21]]): every member over the same samples idx (or 0 .. n-1), member m
        at qps[m]; LDP: qps[m] = -1 puts sample i at slot mixed_eval_slots(seed of m, n)[i]"""
        qps = [int(q) for q in qps]
        if len(qps) != self.k:
            raise ValueError("%d QPs for %d members" % (len(qps), self.k))
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            n = idx.size
        probs = np.empty((self.k, int(n), NOUT), dtype=np.float32) if want_probs else None
        l3, a3 = np.zeros((self.k, 3), np.float32), np.zeros((self.k, 3), np.float32)
        self._chk(self.lib.ethcnn_train_group_evaluate(self.h, int(which), None if idx is None else idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                       int(n), (ctypes.c_int * self.k)(*qps), l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp),
                                                       None if probs is None else probs.ctypes.data_as(_fp)))
        return (l3, a3, probs) if want_probs else (l3, a3)

    def debug_fetch(self, m, which):
        n = {TDBG_GRADS: BLOB_FLOATS, TDBG_ACCUM: BLOB_FLOATS, TDBG_MASK_FC1: self.batch * NVEC, TDBG_MASK_FC2: self.batch * NFC2,
             TDBG_PROBS: self.batch * NOUT, TDBG_INDICES: self.batch * 2, TDBG_H1: self.batch * NVEC}[which]
        out = np.empty(n, dtype=np.float32)
        self._chk(self.lib.ethcnn_train_group_debug_fetch(self.h, int(m), int(which), out.ctypes.data_as(_fp), n))
        return out


# ------------------------------------------------------------------------------------------------------------ sample sets ---
SAMPLES_AI, SAMPLES_INTER = 0, 1
ORDER_ENCODE, ORDER_RA = 0, 1
SAMPLE_BYTES = {SAMPLES_AI: 4992, SAMPLES_INTER: 16516}
PERMUTE_STREAM = 7


def _draw(seed, stream, step, slot, unit):
    return _mix64(_mix64(_mix64((seed ^ stream * 0xD1B54A32D192ED03) & _M64) ^ step) ^ ((slot << 12 | unit) & _M64))


def sample_permutation(seed, count):
    """perm(0 .. count-1) of include/ethcnn.h "sample sets": shuffled record j is record perm[j]"""
    seed, count = int(seed) & _M64, int(count)
    half = 1
    while 4 ** half < count:
        half += 1
    mask = (1 << half) - 1
    out = np.empty(count, dtype=np.int64)
    for j in range(count):
        x = j
        while True:
            l, r = x >> half, x & mask
            for rnd in range(4):
                l, r = r, l ^ (_draw(seed, PERMUTE_STREAM, count, r, rnd) & mask)
            x = l << half | r
            if x < count:
                break
        out[j] = x
    return out


def cut_device(ctx, kind, qps, width, height, nframes, d_luma, pitch, frame_stride, d_labels, d_records, record_offset=0, frame_number=0,
               seq_number=0):
    """ethcnn_samples_cut_device: the cut kernel on frames in HBM.  d_luma / pitch / frame_stride: one entry (All-Intra) or four
    (inter slots); d_labels: one device address per QP; all addresses as integers (DeviceBuffer.ptr.value plus an offset)."""
    n, nq = len(d_luma), len(qps)
    rc = ctx.lib.ethcnn_samples_cut_device(ctx.h, int(kind), (ctypes.c_int * nq)(*[int(q) for q in qps]), nq, int(width), int(height),
                                           int(nframes), (_vp * n)(*[int(p) for p in d_luma]), (_pd * n)(*[int(p) for p in pitch]),
                                           (_pd * n)(*[int(p) for p in frame_stride]), (_vp * nq)(*[int(p) for p in d_labels]),
                                           int(frame_number), int(seq_number), int(d_records), int(record_offset))
    if rc:
        raise EthCnnError(rc, ctx.lib.ethcnn_last_error(ctx.h).decode())


def cut16_device(ctx, qps, width, height, nframes, d_luma16, bit_depth, d_labels, d_records, pitch_bytes=None, frame_stride_bytes=None,
                 record_offset=0):
    """ethcnn_samples_cut16_device: the All-Intra cut kernel on 16-bit luma planes in HBM, narrowed by the rule of include/ethcnn.h while
    they are cut.  pitch_bytes defaults to 2 * width, frame_stride_bytes to height * pitch_bytes; addresses as integers."""
    nq = len(qps)
    pitch_bytes = 2 * int(width) if pitch_bytes is None else int(pitch_bytes)
    frame_stride_bytes = int(height) * pitch_bytes if frame_stride_bytes is None else int(frame_stride_bytes)
    rc = ctx.lib.ethcnn_samples_cut16_device(ctx.h, (ctypes.c_int * nq)(*[int(q) for q in qps]), nq, int(width), int(height), int(nframes),
                                             int(d_luma16), pitch_bytes, frame_stride_bytes, int(bit_depth),
                                             (_vp * nq)(*[int(p) for p in d_labels]), int(d_records), int(record_offset))
    if rc:
        raise EthCnnError(rc, ctx.lib.ethcnn_last_error(ctx.h).decode())


class SampleSet(object):
    """The trainers' sample records, cut out of YUV and label files into HBM (include/ethcnn.h "sample sets").
    kind "ai": 4992-byte records from one YUV and one *_CUDepth.dat per QP; kind "inter" (LDP / LDB / RA): 16516-byte records from four
    residual YUVs and four label files, order="ra" for the Random-Access frame table.  ctx=None validates and counts only."""

    def __init__(self, ctx, kind="ai", qps=(22, 27, 32, 37), order="encode", max_bytes=0, lib=None):
        self.ctx, self.lib = ctx, (ctx.lib if ctx is not None else (lib or load_library()))
        kinds, orders = {"ai": SAMPLES_AI, "inter": SAMPLES_INTER}, {"encode": ORDER_ENCODE, "ra": ORDER_RA}
        self.kind = kinds[kind] if kind in kinds else int(kind)
        self.qps = [int(q) for q in qps]
        h = ctypes.c_void_p()
        rc = self.lib.ethcnn_samples_create(ctx.h if ctx is not None else None, self.kind, (ctypes.c_int * len(self.qps))(*self.qps),
                                            len(self.qps), orders[order] if order in orders else int(order), int(max_bytes), ctypes.byref(h))
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_last_error(ctx.h).decode() if ctx is not None else "bad sample-set arguments")
        self.h = h
        if ctx is not None:
            if not hasattr(ctx, "_trainers"):
                ctx._trainers = weakref.WeakSet()
            ctx._trainers.add(self)  # closed with the context, before it

    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_samples_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_samples_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_source_format(self, bit_depth=8, chroma=420):
        """the source format of the sequences added next (ethcnn_samples_set_source_format; All-Intra sets)"""
        fmt = SourceFormat(int(bit_depth), int(chroma))
        self._chk(self.lib.ethcnn_samples_set_source_format(self.h, ctypes.addressof(fmt)))

    def add_sequence(self, width, height, yuv, labels, bit_depth=8, chroma=420):
        """yuv: the YUV path (All-Intra) or the four residual paths; labels: one *_CUDepth.dat path per QP, in QP-list order;
        bit_depth / chroma: the YUV's source format (bit_depth 8..16, chroma 400 / 420 / 422 / 444; All-Intra sets only)"""
        self.set_source_format(bit_depth, chroma)
        yuv = [yuv] if isinstance(yuv, (str, bytes, os.PathLike)) else list(yuv)
        y = [os.fsencode(p) for p in yuv]
        lab = [os.fsencode(p) for p in labels]
        self._chk(self.lib.ethcnn_samples_add_sequence(self.h, int(width), int(height), (ctypes.c_char_p * len(y))(*y), len(y),
                                                       (ctypes.c_char_p * len(lab))(*lab), len(lab)))

    @property
    def count(self):
        return int(self.lib.ethcnn_samples_count(self.h))

    def __len__(self):
        return self.count

    @property
    def record_bytes(self):
        return int(self.lib.ethcnn_samples_record_bytes(self.h))

    def build(self):
        self._chk(self.lib.ethcnn_samples_build(self.h))
        return self

    def read(self, first=0, n=None, seed=None):
        """records [first, first + n) as a uint8 array [n, record_bytes]; seed: of the set permuted by that seed"""
        n = self.count - first if n is None else int(n)
        out = np.empty((n, self.record_bytes), dtype=np.uint8)
        self._chk(self.lib.ethcnn_samples_read(self.h, int(first), n, 0 if seed is None else 1, 0 if seed is None else int(seed) & _M64,
                                               out.ctypes.data if n else None))
        return out

    def write(self, path, seed=None):
        """the set as a sample file; seed: the "_shuffled" form, permuted by that seed"""
        self._chk(self.lib.ethcnn_samples_write(self.h, os.fsencode(path), 0 if seed is None else 1, 0 if seed is None else int(seed) & _M64))


# ------------------------------------------------------------------------------------------------------- ETH-LSTM training ---
LSTM_SAMPLE_BYTES = 37264  # 64 info bytes + 20 slots of 465 float32 [qp | 16 labels | 448 vector]
LSTM_STEPS, LSTM_SLOT_FLOATS = 20, 465
(LDBG_GRADS, LDBG_NORM, LDBG_ACCUM, LDBG_MASK_H, LDBG_MASK_FC2, LDBG_PROBS, LDBG_INDICES, LDBG_STATE_C, LDBG_STATE_H) = range(9)


class LstmTrainOptions(ctypes.Structure):
    _fields_ = [("batch", ctypes.c_int), ("lr_init", ctypes.c_float), ("momentum", ctypes.c_float), ("decay_rate", ctypes.c_float),
                ("decay_steps", ctypes.c_int64), ("dropout", ctypes.c_int), ("seed", ctypes.c_uint64), ("qp_scale", ctypes.c_float),
                ("clip_norm", ctypes.c_float), ("reserved", ctypes.c_int * 6)]


def lstm_select_qp(records, qps):
    """indices of the 37264-byte samples whose slot-0 QP is in qps (SELECT_QP_LIST, input_data.py:126-134): what
    LstmTrainer.set_samples keeps after set_qps(qps), in this order"""
    raw = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray)) else np.asarray(records, np.uint8)
    q0 = np.ascontiguousarray(raw.reshape(-1, LSTM_SAMPLE_BYTES)[:, 64:68]).view(np.float32)[:, 0]
    return np.arange(q0.size) if not len(qps) else np.flatnonzero(np.isin(q0, np.asarray(qps, np.float32)))


class LstmTrainer(object):
    """ETH-LSTM training on the GPU of an EthCnn context (include/ethcnn.h "ETH-LSTM training").  Defaults are the reference's
    (train_LSTM_CTU64.py:42-52): batch 64, lr 0.1 decayed by 0.3163 every 25000 steps, momentum 0.9, global-norm clip 5, dropout on.
    qp_scale: 1.0 is the training script as shipped; 0.18 trains a model for lstm_step / the LDP daemons."""

    def __init__(self, ctx, batch=64, lr=0.1, momentum=0.9, decay_rate=0.3163, decay_steps=25000, dropout=True, seed=0, qp_scale=1.0,
                 clip_norm=5.0):
        self.ctx, self.lib, self.batch, self.seed = ctx, ctx.lib, int(batch), int(seed) & (2 ** 64 - 1)
        o = LstmTrainOptions(int(batch), float(lr), float(momentum), float(decay_rate), int(decay_steps), 1 if dropout else 0,
                             self.seed, float(qp_scale), float(clip_norm))
        h = ctypes.c_void_p()
        rc = self.lib.ethcnn_lstm_train_create(ctx.h, ctypes.byref(o), ctypes.byref(h))
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_last_error(ctx.h).decode())
        self.h = h
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)

    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_lstm_train_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_lstm_train_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def init_weights(self, seed):
        self._chk(self.lib.ethcnn_lstm_train_init_weights(self.h, int(seed) & (2 ** 64 - 1)))

    def set_blob(self, blob, accum=None):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        acc = None if accum is None else np.ascontiguousarray(accum, dtype=np.float32)
        if acc is not None and acc.size != blob.size:
            raise ValueError("accumulators and blob differ in size")
        self._chk(self.lib.ethcnn_lstm_train_set_blob(self.h, blob.ctypes.data_as(_fp),
                                                      None if acc is None else acc.ctypes.data_as(_fp), blob.size))

    def get_blob(self, with_accum=False):
        blob = np.empty(LSTM_BLOB_FLOATS, dtype=np.float32)
        acc = np.empty(LSTM_BLOB_FLOATS, dtype=np.float32) if with_accum else None
        self._chk(self.lib.ethcnn_lstm_train_get_blob(self.h, blob.ctypes.data_as(_fp),
                                                      None if acc is None else acc.ctypes.data_as(_fp), LSTM_BLOB_FLOATS))
        return (blob, acc) if with_accum else blob

    def set_qps(self, qps):
        """SELECT_QP_LIST for the uploads that follow ([] keeps every sample)"""
        arr = (ctypes.c_int * max(1, len(qps)))(*[int(q) for q in qps])
        self._chk(self.lib.ethcnn_lstm_train_set_qps(self.h, arr, len(qps)))

    def set_samples(self, which, records, take=False):
        """records: bytes / uint8 array of whole 37264-byte samples (get_LSTM_input.py's output), or a built LstmSampleSet, which
        stays in HBM (take=True: the set is empty afterwards, and the trainer adopts its buffer when the QP selection keeps every
        sample; else a device-to-device copy of the kept samples); returns the number kept"""
        if isinstance(records, LstmSampleSet):
            self._chk(self.lib.ethcnn_lstm_train_set_samples_from(self.h, int(which), records.h, 1 if take else 0))
            return self.num_samples(which)
        buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records, np.uint8)
        self._chk(self.lib.ethcnn_lstm_train_set_samples(self.h, int(which), buf.ctypes.data if buf.size else None, buf.size))
        return self.num_samples(which)

    def num_samples(self, which):
        return int(self.lib.ethcnn_lstm_train_num_samples(self.h, int(which)))

    def run(self, first_step, nsteps):
        """enqueue steps first_step .. first_step + nsteps - 1 (device-drawn batches); returns at once"""
        self._chk(self.lib.ethcnn_lstm_train_run(self.h, int(first_step), int(nsteps)))

    def last_stats(self):
        l3, a3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._chk(self.lib.ethcnn_lstm_train_last_stats(self.h, l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp)))
        return l3, a3

    def step_indices(self, step, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        l3, a3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._chk(self.lib.ethcnn_lstm_train_step_indices(self.h, int(step), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), idx.size,
                                                          l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp)))
        return l3, a3

    def evaluate(self, which, idx=None, n=None, want_probs=False):
        """(loss_list, accuracy_list[, probs [20 n, 21]]) of ONE forward batch over the samples idx (or 0 .. n-1); rows 20 i + p"""
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            n = idx.size
        if n is None:
            raise ValueError("evaluate needs idx or n")
        probs = np.empty((int(n) * LSTM_STEPS, NOUT), dtype=np.float32) if want_probs else None
        l3, a3 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._chk(self.lib.ethcnn_lstm_train_evaluate(self.h, int(which),
                                                      None if idx is None else idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(n),
                                                      l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp),
                                                      None if probs is None else probs.ctypes.data_as(_fp)))
        return (l3, a3, probs) if want_probs else (l3, a3)

    def debug_fetch(self, which):
        rows = int(self.lib.ethcnn_lstm_train_debug_rows(self.h))  # of the last step / the last piece of the last evaluation
        n = {LDBG_GRADS: LSTM_BLOB_FLOATS, LDBG_ACCUM: LSTM_BLOB_FLOATS, LDBG_NORM: 1, LDBG_MASK_H: rows * NVEC,
             LDBG_MASK_FC2: rows * NFC2, LDBG_PROBS: self.batch * LSTM_STEPS * NOUT, LDBG_INDICES: rows // LSTM_STEPS,
             LDBG_STATE_C: rows * NVEC, LDBG_STATE_H: rows * NVEC}.get(which, 1)
        out = np.empty(n, dtype=np.float32)
        self._chk(self.lib.ethcnn_lstm_train_debug_fetch(self.h, int(which), out.ctypes.data_as(_fp), n))
        return out


def lstm_train_options(batch=64, lr=0.1, momentum=0.9, decay_rate=0.3163, decay_steps=25000, dropout=True, seed=0, qp_scale=1.0,
                       clip_norm=5.0):
    """the LstmTrainOptions of LstmTrainer's keyword arguments (an LstmTrainerGroup takes a list of them)"""
    return LstmTrainOptions(int(batch), float(lr), float(momentum), float(decay_rate), int(decay_steps), 1 if dropout else 0,
                            int(seed) & _M64, float(qp_scale), float(clip_norm))


def _lstm_train_options_array(opts):
    opts = list(opts)
    for o in opts:
        if not isinstance(o, LstmTrainOptions):
            raise TypeError("an LSTM trainer group takes LstmTrainOptions, got %r" % type(o).__name__)
    return (LstmTrainOptions * max(len(opts), 1))(*opts), len(opts)


def lstm_train_group_check(opts, lib=None):
    """host-only check of an LSTM trainer group's options (no context): raises EthCnnError(ERR_ARG) naming the member and the field"""
    lib = lib or load_library()
    arr, k = _lstm_train_options_array(opts)
    err = ctypes.create_string_buffer(256)
    rc = lib.ethcnn_lstm_train_group_check(arr, k, err, len(err))
    if rc:
        raise EthCnnError(rc, err.value.decode())


def lstm_group_keep_list(records, qps, lib=None):
    """host only: the records (file order) an LstmTrainerGroup member with the QP list `qps` keeps of a sample file -- the library's
    own selection, equal to lstm_select_qp(records, qps)"""
    lib = lib or load_library()
    buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records, np.uint8)
    keep = np.empty(max(buf.size // LSTM_SAMPLE_BYTES, 1), np.int64)
    n = ctypes.c_int64()
    arr = (ctypes.c_int * max(1, len(qps)))(*[int(q) for q in qps])
    rc = lib.ethcnn_lstm_train_group_keep_list(buf.ctypes.data if buf.size else None, buf.size, arr, len(qps),
                                               keep.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(n))
    if rc:
        raise EthCnnError(rc, "%d bytes is not a whole number of %d-byte samples, or a bad QP list" % (buf.size, LSTM_SAMPLE_BYTES))
    return keep[:n.value].copy()


class LstmTrainerGroup(object):
    """K (1..8) independent ETH-LSTM trainers in every launch of a step (include/ethcnn.h "ETH-LSTM training, several models at
    once"): one context, one stream, one copy of the sample sets.  Member m computes what LstmTrainer computes with opts[m], its QP
    list and its own upload of the same samples, bit for bit.  opts: a list of LstmTrainOptions (lstm_train_options(...)) with the
    same batch.  Sample indices of member m count the samples m keeps."""

    def __init__(self, ctx, opts):
        self.ctx, self.lib = ctx, ctx.lib
        arr, k = _lstm_train_options_array(opts)
        h = ctypes.c_void_p()
        rc = self.lib.ethcnn_lstm_train_group_create(ctx.h, arr, k, ctypes.byref(h))
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_last_error(ctx.h).decode())
        self.h, self.k, self.batch = h, k, int(arr[0].batch)
        self.seeds = [int(arr[m].seed) for m in range(k)]
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)

    def __len__(self):
        return self.k

    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_lstm_train_group_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_lstm_train_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def init_weights(self, seeds):
        """seeds: one per member, or one number for all"""
        seeds = [seeds] * self.k if np.isscalar(seeds) else list(seeds)
        if len(seeds) != self.k:
            raise ValueError("%d seeds for %d members" % (len(seeds), self.k))
        self._chk(self.lib.ethcnn_lstm_train_group_init_weights(self.h, (ctypes.c_uint64 * self.k)(*[int(x) & _M64 for x in seeds])))

    def set_blob(self, m, blob, accum=None):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        acc = None if accum is None else np.ascontiguousarray(accum, dtype=np.float32)
        if acc is not None and acc.size != blob.size:
            raise ValueError("accumulators and blob differ in size")
        self._chk(self.lib.ethcnn_lstm_train_group_set_blob(self.h, int(m), blob.ctypes.data_as(_fp),
                                                            None if acc is None else acc.ctypes.data_as(_fp), blob.size))

    def get_blob(self, m, with_accum=False):
        blob = np.empty(LSTM_BLOB_FLOATS, dtype=np.float32)
        acc = np.empty(LSTM_BLOB_FLOATS, dtype=np.float32) if with_accum else None
        self._chk(self.lib.ethcnn_lstm_train_group_get_blob(self.h, int(m), blob.ctypes.data_as(_fp),
                                                            None if acc is None else acc.ctypes.data_as(_fp), LSTM_BLOB_FLOATS))
        return (blob, acc) if with_accum else blob

    def set_qps(self, m, qps):
        """SELECT_QP_LIST of member m for the uploads that follow ([] keeps every sample)"""
        arr = (ctypes.c_int * max(1, len(qps)))(*[int(q) for q in qps])
        self._chk(self.lib.ethcnn_lstm_train_group_set_qps(self.h, int(m), arr, len(qps)))

    def set_samples(self, which, records, take=False):
        """what LstmTrainer.set_samples takes; one copy in HBM serves every member (take=True: an LstmSampleSet's buffer is adopted
        and the set is empty afterwards); returns the number of samples each member keeps"""
        if isinstance(records, LstmSampleSet):
            self._chk(self.lib.ethcnn_lstm_train_group_set_samples_from(self.h, int(which), records.h, 1 if take else 0))
        else:
            buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records, np.uint8)
            self._chk(self.lib.ethcnn_lstm_train_group_set_samples(self.h, int(which), buf.ctypes.data if buf.size else None, buf.size))
        return [self.num_samples(m, which) for m in range(self.k)]

    def num_samples(self, m, which):
        return int(self.lib.ethcnn_lstm_train_group_num_samples(self.h, int(m), int(which)))

    def run(self, first_step, nsteps):
        """enqueue steps first_step .. first_step + nsteps - 1 of every member (device-drawn batches); returns at once"""
        self._chk(self.lib.ethcnn_lstm_train_group_run(self.h, int(first_step), int(nsteps)))

    def last_stats(self):
        """(loss_list [k,3], accuracy_list [k,3]) of the last step enqueued (waits for it)"""
        l3, a3 = np.zeros((self.k, 3), np.float32), np.zeros((self.k, 3), np.float32)
        self._chk(self.lib.ethcnn_lstm_train_group_last_stats(self.h, l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp)))
        return l3, a3

    def step_indices(self, step, idx):
        """idx [k, batch], row m in member m's own kept indices"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.shape != (self.k, self.batch):
            raise ValueError("idx must be [%d, %d]" % (self.k, self.batch))
        l3, a3 = np.zeros((self.k, 3), np.float32), np.zeros((self.k, 3), np.float32)
        self._chk(self.lib.ethcnn_lstm_train_group_step_indices(self.h, int(step), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                                self.batch, l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp)))
        return l3, a3

    def evaluate(self, which, idx=None, n=None, want_probs=False):
        """(loss_list [k,3], accuracy_list [k,3][, probs [k, 20 n, 21]]): member m over its samples idx[m] (idx [k, n], its own kept
        indices) or, idx None, its samples 0 .. n-1; per member ONE forward batch"""
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            if idx.ndim != 2 or idx.shape[0] != self.k:
                raise ValueError("idx must be [%d, n]" % self.k)
            n = idx.shape[1]
        if n is None:
            raise ValueError("evaluate needs idx or n")
        probs = np.empty((self.k, int(n) * LSTM_STEPS, NOUT), dtype=np.float32) if want_probs else None
        l3, a3 = np.zeros((self.k, 3), np.float32), np.zeros((self.k, 3), np.float32)
        self._chk(self.lib.ethcnn_lstm_train_group_evaluate(self.h, int(which),
                                                            None if idx is None else idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                            int(n), l3.ctypes.data_as(_fp), a3.ctypes.data_as(_fp),
                                                            None if probs is None else probs.ctypes.data_as(_fp)))
        return (l3, a3, probs) if want_probs else (l3, a3)

    def debug_fetch(self, m, which):
        rows = int(self.lib.ethcnn_lstm_train_group_debug_rows(self.h, int(m)))
        n = {LDBG_GRADS: LSTM_BLOB_FLOATS, LDBG_ACCUM: LSTM_BLOB_FLOATS, LDBG_NORM: 1, LDBG_MASK_H: rows * NVEC,
             LDBG_MASK_FC2: rows * NFC2, LDBG_PROBS: self.batch * LSTM_STEPS * NOUT, LDBG_INDICES: rows // LSTM_STEPS,
             LDBG_STATE_C: rows * NVEC, LDBG_STATE_H: rows * NVEC}.get(which, 1)
        out = np.empty(n, dtype=np.float32)
        self._chk(self.lib.ethcnn_lstm_train_group_debug_fetch(self.h, int(m), int(which), out.ctypes.data_as(_fp), n))
        return out


# ------------------------------------------------------------------------------------------------- ETH-LSTM sample sets ---
LDP_RECORD_BYTES = 16516


def lstm_samples_plan(records, lib=None):
    """ethcnn_lstm_samples_plan on uint8 LDP records (host only): (heads [m], strides [m], skipped); time slot k of head j is record
    heads[j] - k * strides[j]"""
    lib = lib or load_library()
    buf = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records, np.uint8)
    n = buf.size // LDP_RECORD_BYTES
    heads, strides = np.empty(max(n, 1), np.int64), np.empty(max(n, 1), np.int64)
    m, skipped = ctypes.c_int64(), ctypes.c_int64()
    p64 = ctypes.POINTER(ctypes.c_int64)
    rc = lib.ethcnn_lstm_samples_plan(buf.ctypes.data if buf.size else None, buf.size, heads.ctypes.data_as(p64), strides.ctypes.data_as(p64),
                                      ctypes.byref(m), ctypes.byref(skipped))
    if rc:
        raise EthCnnError(rc, "%d bytes is not a whole number of %d-byte records" % (buf.size, LDP_RECORD_BYTES))
    return heads[:m.value].copy(), strides[:m.value].copy(), int(skipped.value)


class LstmSampleSet(object):
    """The ETH-LSTM trainer's 37264-byte samples, built in HBM from Low-Delay-P records with the residual CNN the context has loaded
    (include/ethcnn.h "ETH-LSTM sample sets"): what get_LSTM_input.build_samples returns.  slots: the QP slots (0..3) to build, None =
    all four; chunk_ctus: records per pass through the CNN (0 = default)."""

    def __init__(self, ctx, slots=None, chunk_ctus=0, max_bytes=0):
        self.ctx, self.lib = ctx, ctx.lib
        sl = [] if slots is None else [int(q) for q in slots]
        h = ctypes.c_void_p()
        rc = self.lib.ethcnn_lstm_samples_create(ctx.h, (ctypes.c_int * max(1, len(sl)))(*sl), len(sl), int(chunk_ctus), int(max_bytes),
                                                 ctypes.byref(h))
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_last_error(ctx.h).decode())
        self.h = h
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)  # closed with the context, before it

    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_lstm_samples_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_lstm_samples_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def build_from(self, x):
        """x: a built inter SampleSet (read in HBM, left as it is), a uint8 array / bytes of 16516-byte records, or the path of a
        file of them"""
        if isinstance(x, SampleSet):
            self._chk(self.lib.ethcnn_lstm_samples_build_from_set(self.h, x.h))
            return self
        if isinstance(x, (str, os.PathLike)):
            x = np.memmap(x, dtype=np.uint8, mode="r") if os.path.getsize(x) else np.empty(0, np.uint8)
        buf = np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8)
        self._chk(self.lib.ethcnn_lstm_samples_build_from_records(self.h, buf.ctypes.data if buf.size else None, buf.size))
        return self

    @property
    def count(self):
        return int(self.lib.ethcnn_lstm_samples_count(self.h))

    @property
    def skipped(self):
        return int(self.lib.ethcnn_lstm_samples_skipped(self.h))

    def __len__(self):
        return self.count

    def read(self, first=0, n=None):
        """samples [first, first + n) as a uint8 array [n, 37264]"""
        n = self.count - first if n is None else int(n)
        out = np.empty((n, LSTM_SAMPLE_BYTES), dtype=np.uint8)
        self._chk(self.lib.ethcnn_lstm_samples_read(self.h, int(first), n, out.ctypes.data if n else None))
        return out

    def write(self, path):
        self._chk(self.lib.ethcnn_lstm_samples_write(self.h, os.fsencode(path)))


# ------------------------------------------------------------------------------------------------------------ calibration ---
CALIB_BINS, CALIB_LEVELS = 1025, 3
THR_ORDER_AI, THR_ORDER_LDP = 0, 1
_THR_ORDERS = {"ai": THR_ORDER_AI, "ldp": THR_ORDER_LDP}


class CalibLevel(ctypes.Structure):
    _fields_ = [("n0", ctypes.c_uint64), ("n1", ctypes.c_uint64), ("down_k", ctypes.c_int32), ("up_k", ctypes.c_int32),
                ("down", ctypes.c_double), ("up", ctypes.c_double), ("miss", ctypes.c_uint64), ("fsplit", ctypes.c_uint64),
                ("uncertain", ctypes.c_uint64), ("uncertain_share", ctypes.c_double), ("accuracy_512", ctypes.c_double),
                ("empty_class", ctypes.c_int32), ("crossed", ctypes.c_int32)]


class CalibReport(ctypes.Structure):
    _fields_ = [("level", CalibLevel * 3)]

    def as_dicts(self):
        return [{name: getattr(lv, name) for name, _ in CalibLevel._fields_} for lv in self.level]


def _ppm3(eps):
    eps = [int(e) for e in (eps if hasattr(eps, "__len__") else (eps,) * 3)]
    if len(eps) != 3 or min(eps) < 0 or max(eps) > 1000000:
        raise ValueError("a budget is three values in parts per million, 0..1000000: %r" % (eps,))
    return (ctypes.c_uint32 * 3)(*eps)


def calib_choose(hist, eps_down_ppm, eps_up_ppm, lib=None):
    """ethcnn_calib_choose (host only): hist uint64 [3, 2, 1025], budgets in parts per million (three values, or one for all levels)
    -> CalibReport"""
    lib = lib or load_library()
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    if hist.size != CALIB_LEVELS * 2 * CALIB_BINS:
        raise ValueError("a histogram holds 3 x 2 x 1025 counts, got %d" % hist.size)
    rep = CalibReport()
    rc = lib.ethcnn_calib_choose(hist.ctypes.data, _ppm3(eps_down_ppm), _ppm3(eps_up_ppm), ctypes.byref(rep))
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return rep


def write_thr_info(path, report, order, lib=None):
    """ethcnn_calib_write_thr_info (host only).  order "ai": up1 down1 up2 down2 up3 down3 (TEncCu.cpp:250 of HM-16.5_Test_AI);
    "ldp": down1 up1 down2 up2 down3 up3 (TEncGOP.cpp:1449 of HM-16.5_Test_LDP)."""
    lib = lib or load_library()
    if order not in _THR_ORDERS:
        raise ValueError("order is 'ai' or 'ldp', got %r" % (order,))
    rc = lib.ethcnn_calib_write_thr_info(os.fsencode(path), ctypes.byref(report), _THR_ORDERS[order])
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())


class Calibrator(object):
    """Per-level histograms of the split probabilities by ground truth, counted on the GPU, and the Thr_info.txt thresholds chosen
    from them (include/ethcnn.h "threshold calibration").  The probabilities must come from a prediction with OPEN gates
    (set_thresholds(0, 0)): the batch gates zero whole sub-batches of p32 / p16."""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib
        h = ctypes.c_void_p()
        ctx._chk(self.lib.ethcnn_calib_create(ctx.h, ctypes.byref(h)))
        self.h = h
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)  # closed with the context, before it

    def _chk(self, rc):
        self.ctx._chk(rc)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_calib_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        self._chk(self.lib.ethcnn_calib_reset(self.h))

    def add(self, probs, depth16):
        """probs float32 [n, 21], depth16 uint8 [n, 16] (a sample's label bytes) in host memory"""
        probs = np.ascontiguousarray(probs, dtype=np.float32).reshape(-1, NOUT)
        depth16 = np.ascontiguousarray(depth16, dtype=np.uint8).reshape(-1, 16)
        if probs.shape[0] != depth16.shape[0]:
            raise ValueError("%d rows of probabilities, %d of depths" % (probs.shape[0], depth16.shape[0]))
        n = probs.shape[0]
        self._chk(self.lib.ethcnn_calib_add(self.h, probs.ctypes.data if n else None, depth16.ctypes.data if n else None, n))

    def add_device(self, d_probs, d_depth16, n):
        """the same on buffers in HBM (DeviceBuffer or raw device addresses)"""
        ptr = lambda b: getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_calib_add_device(self.h, ptr(d_probs), ptr(d_depth16), int(n)))

    @staticmethod
    def _frames(width, height, nprobs, nlabels, nframes, skip):
        if width % 16 or height % 16 or width <= 0 or height <= 0:
            return None  # the library names the error
        per, lab = ctus_per_frame(width, height) * NOUT, (width // 16) * (height // 16)
        if nframes is None:
            if nprobs % per:
                raise ValueError("%d probabilities are not a whole number of %dx%d frames" % (nprobs, width, height))
            nframes = nprobs // per
        if nprobs < nframes * per or nlabels < (nframes + skip) * lab:
            raise ValueError("%d frames (+ %d skipped label frames) need %d probabilities and %d label bytes, got %d and %d"
                             % (nframes, skip, nframes * per, (nframes + skip) * lab, nprobs, nlabels))
        return nframes

    def add_frames(self, probs, labels, width, height, skip_label_frames=0, nframes=None):
        """probs float32 [frames, nctu, 21] (a cu_depth.dat), labels uint8 [skip + frames, height / 16, width / 16] (an
        Info_*_CUDepth.dat) in host memory; CTUs that are not wholly inside the picture are left out (skipped_partial)"""
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        nf = self._frames(width, height, probs.size, labels.size, nframes, int(skip_label_frames))
        self._chk(self.lib.ethcnn_calib_add_frames(self.h, probs.ctypes.data if probs.size else None, labels.ctypes.data if labels.size else None,
                                                   int(width), int(height), 0 if nf is None else nf, int(skip_label_frames)))

    def add_frames_device(self, d_probs, d_labels, width, height, nframes, skip_label_frames=0):
        """the same on buffers in HBM, e.g. the output ldp_sequence_device left there"""
        ptr = lambda b: getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_calib_add_frames_device(self.h, ptr(d_probs), ptr(d_labels), int(width), int(height), int(nframes),
                                                          int(skip_label_frames)))

    def get(self):
        """(hist uint64 [3, 2, 1025] = [level, truth, bin], rejected uint64 [3], skipped_partial); waits for the stream"""
        hist, rej, sk = np.zeros((CALIB_LEVELS, 2, CALIB_BINS), np.uint64), np.zeros(3, np.uint64), ctypes.c_uint64(0)
        self._chk(self.lib.ethcnn_calib_get(self.h, hist.ctypes.data, rej.ctypes.data, ctypes.byref(sk)))
        return hist, rej, int(sk.value)

    def histogram(self):
        return self.get()[0]

    def choose(self, eps_down_ppm, eps_up_ppm):
        return calib_choose(self.histogram(), eps_down_ppm, eps_up_ppm, self.lib)

    def write_thr_info(self, path, report, order):
        write_thr_info(path, report, order, self.lib)


# ------------------------------------------------------------------------------------------------------------- simulation ---
SIM_GATES_NONE, SIM_GATES_AI, SIM_GATES_LDP = 0, 1, 2
_SIM_GATES = {"none": SIM_GATES_NONE, "ai": SIM_GATES_AI, "ldp": SIM_GATES_LDP}
SIM_COORDS = ("down0", "up0", "down1", "up1", "down2", "up2")
# ethcnn_sim_thr / ethcnn_sim_counts as numpy records
SIM_THR = np.dtype([("up_k", "<i4", (3,)), ("down_k", "<i4", (3,))])
SIM_COUNTS = np.dtype([("checked", "<u8", (4,)), ("split_only", "<u8", (3,)), ("current_only", "<u8", (3,)), ("both", "<u8", (3,)),
                       ("edge_split", "<u8", (3,)), ("wrong_split", "<u8", (3,)), ("wrong_stop", "<u8", (3,)), ("bad_ctus", "<u8")])
SIM_FULL_SEARCH = ((1024, 1024, 1024), (-1, -1, -1))
REACH_MAX_CAND = 256
# partition decisions: bytes of a codes row, and its flag bits (byte 21)
SIM_CODE_BYTES = 24
SIM_FLAG_BAD, SIM_FLAG_LABELLED, SIM_FLAG_REJECTED, SIM_FLAG_GATE1_CLOSED, SIM_FLAG_GATE2_CLOSED = 1, 2, 4, 8, 16


def sim_thr(up_k, down_k):
    """one candidate (or, from [K, 3] arrays, K of them) as SIM_THR records"""
    up_k, down_k = np.asarray(up_k, dtype=np.int32), np.asarray(down_k, dtype=np.int32)
    out = np.zeros(up_k.shape[:-1], SIM_THR)
    out["up_k"], out["down_k"] = up_k, down_k
    return out


def _sim_cands(cands):
    cands = np.asarray(cands)
    if cands.dtype != SIM_THR:  # [K, 2, 3]: (up_k, down_k) rows
        cands = sim_thr(cands[..., 0, :], cands[..., 1, :])
    return np.ascontiguousarray(cands).reshape(-1)


def sim_write_thr_info(path, thr, order, lib=None):
    """ethcnn_sim_write_thr_info (host only): one SIM_THR record in the line format and token orders of write_thr_info"""
    lib = lib or load_library()
    if order not in _THR_ORDERS:
        raise ValueError("order is 'ai' or 'ldp', got %r" % (order,))
    thr = _sim_cands(thr)
    if thr.size != 1:
        raise ValueError("one candidate makes one Thr_info.txt, got %d" % thr.size)
    rc = lib.ethcnn_sim_write_thr_info(os.fsencode(path), thr.ctypes.data, _THR_ORDERS[order])
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())


def sim_counts_from_codes(codes, lib=None):
    """ethcnn_decide_counts_from_codes (host only): the SIM_COUNTS record of codes uint8 [n, 24] as PartitionSim.decide returns them --
    of the whole set it equals PartitionSim.eval of the same candidate; of a frame's or a sequence's rows it is their share"""
    lib = lib or load_library()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if codes.size % SIM_CODE_BYTES:
        raise ValueError("%d bytes are not whole %d-byte code rows" % (codes.size, SIM_CODE_BYTES))
    out = np.zeros(1, SIM_COUNTS)
    rc = lib.ethcnn_decide_counts_from_codes(codes.ctypes.data if codes.size else None, codes.size // SIM_CODE_BYTES, out.ctypes.data)
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return out[0]


# search budget (include/ethcnn.h "search budget")
BUDGET_FRAME, BUDGET_CARRY = 0, 1
_BUDGET_MODES = {"frame": BUDGET_FRAME, "carry": BUDGET_CARRY}
BUDGET_DEFAULT_RUNGS, BUDGET_MAX_RUNGS = 513, 4096
BUDGET_WEIGHTS = (64, 16, 4, 1)


def budget_default_ladder(lib=None):
    """ethcnn_budget_default_ladder (host only): SIM_THR records [513], rung j = up_k 1024 - j, down_k j - 1 on all levels"""
    lib = lib or load_library()
    out = np.zeros(BUDGET_DEFAULT_RUNGS, SIM_THR)
    rc = lib.ethcnn_budget_default_ladder(out.ctypes.data)
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return out


def budget_companion_thr(lib=None):
    """ethcnn_budget_companion_thr (host only): the SIM_THR record (768, 256 on all levels) of the Thr_info.txt that goes with a baked
    cu_depth.dat; sim_write_thr_info writes it"""
    lib = lib or load_library()
    out = np.zeros(1, SIM_THR)
    rc = lib.ethcnn_budget_companion_thr(out.ctypes.data)
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return out[0]


def _budget_mode(mode):
    if mode not in _BUDGET_MODES:
        raise ValueError("mode is 'frame' or 'carry', got %r" % (mode,))
    return _BUDGET_MODES[mode]


def budget_choose(checked, weights=None, budget_ppm=1000000, mode="frame", lib=None):
    """ethcnn_budget_choose (host only): checked uint32 [F, K + 1, 4] as PartitionSim.budget_cost returns it (column K = the full
    search) -> dict: rung int32 [F], over bool [F], cost uint64 [F], full uint64 [F]"""
    lib = lib or load_library()
    checked = np.ascontiguousarray(checked, dtype=np.uint32)
    if checked.ndim != 3 or checked.shape[1] < 2 or checked.shape[2] != 4:
        raise ValueError("checked is [frames, K + 1, 4], got shape %r" % (checked.shape,))
    nf, k = checked.shape[0], checked.shape[1] - 1
    w = (ctypes.c_uint64 * 4)(*[int(x) for x in (BUDGET_WEIGHTS if weights is None else weights)])
    rung, over = np.zeros(nf, np.int32), np.zeros(nf, np.uint8)
    cost, full = np.zeros(nf, np.uint64), np.zeros(nf, np.uint64)
    rc = lib.ethcnn_budget_choose(checked.ctypes.data if nf else None, nf, k, w, int(budget_ppm), _budget_mode(mode), rung.ctypes.data, over.ctypes.data,
                                  cost.ctypes.data, full.ctypes.data)
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return {"rung": rung, "over": over.astype(bool), "cost": cost, "full": full}


class PartitionSim(object):
    """HM's pruned CU search simulated over a set of predicted CTUs that stays in HBM, for any number of candidate Thr_info files at
    once (include/ethcnn.h "partition-search simulation"): the RD checks that remain per CU size and, with labels, the labelled
    partitions the pruned search can no longer reach.  gates: "none", "ai" or "ldp"."""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib
        h = ctypes.c_void_p()
        ctx._chk(self.lib.ethcnn_sim_create(ctx.h, ctypes.byref(h)))
        self.h = h
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)  # closed with the context, before it

    def _chk(self, rc):
        self.ctx._chk(rc)

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_sim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        self._chk(self.lib.ethcnn_sim_reset(self.h))

    def add(self, probs, depth16=None):
        """probs float32 [n, 21], depth16 uint8 [n, 16] or None, in host memory"""
        probs = np.ascontiguousarray(probs, dtype=np.float32).reshape(-1, NOUT)
        n = probs.shape[0]
        if depth16 is not None:
            depth16 = np.ascontiguousarray(depth16, dtype=np.uint8).reshape(-1, 16)
            if depth16.shape[0] != n:
                raise ValueError("%d rows of probabilities, %d of depths" % (n, depth16.shape[0]))
        self._chk(self.lib.ethcnn_sim_add(self.h, probs.ctypes.data if n else None, depth16.ctypes.data if n and depth16 is not None else None, n))

    def add_device(self, d_probs, d_depth16, n):
        """the same on buffers in HBM (DeviceBuffer or raw device addresses; d_depth16 may be None)"""
        ptr = lambda b: getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_sim_add_device(self.h, ptr(d_probs), ptr(d_depth16), int(n)))

    def add_frames(self, probs, labels, width, height, skip_label_frames=0, nframes=None):
        """probs float32 [frames, nctu, 21] (a cu_depth.dat), labels uint8 [skip + frames, height / 16, width / 16] (an
        Info_*_CUDepth.dat) or None, in host memory; partial CTUs are simulated, labels are used on whole CTUs only"""
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        unit = 8 if labels is None else 16
        nf = 0
        if width > 0 and height > 0 and width % unit == 0 and height % unit == 0:  # (else the library names the error)
            per = ctus_per_frame(width, height) * NOUT
            nf = probs.size // per if nframes is None else int(nframes)
            if (nframes is None and probs.size % per) or probs.size < nf * per:
                raise ValueError("%d probabilities are not %s %dx%d frames" % (probs.size, "whole" if nframes is None else "%d" % nf, width, height))
            if labels is not None:
                labels = np.ascontiguousarray(labels, dtype=np.uint8)
                if labels.size < (nf + int(skip_label_frames)) * (width // 16) * (height // 16):
                    raise ValueError("%d frames (+ %d skipped label frames) need %d label bytes, got %d"
                                     % (nf, skip_label_frames, (nf + int(skip_label_frames)) * (width // 16) * (height // 16), labels.size))
        self._chk(self.lib.ethcnn_sim_add_frames(self.h, probs.ctypes.data if probs.size else None,
                                                 labels.ctypes.data if labels is not None and labels.size else None, int(width), int(height), nf,
                                                 int(skip_label_frames)))

    def add_frames_device(self, d_probs, d_labels, width, height, nframes, skip_label_frames=0):
        """the same on buffers in HBM, e.g. the output ldp_sequence_device left there (d_labels may be None)"""
        ptr = lambda b: getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_sim_add_frames_device(self.h, ptr(d_probs), ptr(d_labels), int(width), int(height), int(nframes),
                                                        int(skip_label_frames)))

    def info(self):
        """dict: ctus, whole_ctus, labelled_ctus, rejected_ctus, sub_batches (all independent of the candidate)"""
        v = (ctypes.c_uint64 * 5)()
        self._chk(self.lib.ethcnn_sim_info(self.h, v))
        return dict(zip(("ctus", "whole_ctus", "labelled_ctus", "rejected_ctus", "sub_batches"), (int(x) for x in v)))

    def eval(self, cands, gates="none"):
        """cands: SIM_THR records, or integers [K, 2, 3] = (up_k, down_k) rows -> SIM_COUNTS records [K]"""
        cands = _sim_cands(cands)
        out = np.zeros(cands.size, SIM_COUNTS)
        self._chk(self.lib.ethcnn_sim_eval(self.h, cands.ctypes.data if cands.size else None, cands.size, _SIM_GATES[gates],
                                           out.ctypes.data if cands.size else None))
        return out

    def sweep(self, base, coord, gates="none"):
        """every value of one coordinate ("down0", "up0", ... or 0..5) around `base` -> (values int32 [m], SIM_COUNTS records [m])"""
        coord = SIM_COORDS.index(coord) if coord in SIM_COORDS else int(coord)
        base = _sim_cands(base)
        out = np.zeros(1026, SIM_COUNTS)
        self._chk(self.lib.ethcnn_sim_sweep(self.h, base.ctypes.data, coord, _SIM_GATES[gates], out.ctypes.data))
        lo = 0 if coord & 1 else -1
        return np.arange(lo, 1025, dtype=np.int32), out[:1025 - lo]

    def search(self, start, gates, weights, max_bad_ppm, max_rounds=16):
        """coordinate descent from `start` -> (SIM_THR record, SIM_COUNTS record, rounds)"""
        start = _sim_cands(start)
        w = (ctypes.c_uint64 * 4)(*[int(x) for x in weights])
        thr, counts, rounds = np.zeros(1, SIM_THR), np.zeros(1, SIM_COUNTS), ctypes.c_int(0)
        self._chk(self.lib.ethcnn_sim_search(self.h, start.ctypes.data, _SIM_GATES[gates], w, int(max_bad_ppm), int(max_rounds), thr.ctypes.data,
                                             counts.ctypes.data, ctypes.byref(rounds)))
        return thr[0], counts[0], rounds.value

    def write_thr_info(self, path, thr, order):
        sim_write_thr_info(path, thr, order, self.lib)

    # --------------------------------------------------------------------------------------------------- partition decisions ---
    @staticmethod
    def _one(thr):
        thr = _sim_cands(thr)
        if thr.size != 1:
            raise ValueError("the decisions are those of one candidate, got %d" % thr.size)
        return thr

    def set_decide_piece(self, ctus=0):
        """CTUs per staged piece of decide() (0: the default)"""
        self._chk(self.lib.ethcnn_decide_set_piece(self.h, int(ctus)))

    def decide(self, thr, gates="none", mid_k=512, first=0, n=None, want=("codes", "reach", "depth")):
        """the decisions of candidate `thr` on CTUs first .. first + n of the set (include/ethcnn.h "partition decisions") -> dict of
        numpy arrays: codes uint8 [n, 24], reach uint8 [n, 16], depth uint8 [n, 16] (those named in `want`)"""
        thr = self._one(thr)
        n = self.info()["ctus"] - int(first) if n is None else int(n)
        out = {"codes": np.zeros((max(n, 0), SIM_CODE_BYTES), np.uint8), "reach": np.zeros((max(n, 0), 16), np.uint8),
               "depth": np.zeros((max(n, 0), 16), np.uint8)}
        out = {k: v for k, v in out.items() if k in want}
        ptr = lambda k: out[k].ctypes.data if k in out and out[k].size else None
        self._chk(self.lib.ethcnn_decide(self.h, thr.ctypes.data, _SIM_GATES[gates], int(mid_k), int(first), n, ptr("codes"), ptr("reach"), ptr("depth")))
        return out

    def decide_device(self, thr, gates, mid_k, first, n, d_codes, d_reach, d_depth):
        """the same into buffers in HBM (DeviceBuffer, raw device address or None): [n, 24], [n, 16], [n, 16] bytes"""
        ptr = lambda b: getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_decide_device(self.h, self._one(thr).ctypes.data, _SIM_GATES[gates], int(mid_k), int(first), int(n), ptr(d_codes),
                                                ptr(d_reach), ptr(d_depth)))

    def decide_frames_device(self, thr, gates, mid_k, first, width, height, nframes, d_codes, d_reach, d_planes):
        """the frame form into buffers in HBM: whole frames from CTU `first` on, which were added as width x height frames; d_planes
        [nframes, height / 16, width / 16] takes the preferred partition as label planes"""
        ptr = lambda b: getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_decide_frames_device(self.h, self._one(thr).ctypes.data, _SIM_GATES[gates], int(mid_k), int(first), int(width),
                                                       int(height), int(nframes), ptr(d_codes), ptr(d_reach), ptr(d_planes)))

    def decide_frames(self, thr, gates, width, height, first_frame=0, nframes=None, mid_k=512, first=0, planes=True):
        """frames first_frame .. + nframes (default: to the end of the set) of the CTUs added as width x height frames from CTU `first`
        on -> dict: codes uint8 [nframes * nctu, 24], reach uint8 [nframes * nctu, 16] and, with planes, planes uint8 [nframes,
        height / 16, width / 16]: the preferred partition in the layout of an Info_*_CUDepth.dat"""
        width, height = int(width), int(height)
        if width <= 0 or height <= 0:
            raise ValueError("got %d x %d" % (width, height))
        per = ctus_per_frame(width, height)
        at = int(first) + int(first_frame) * per
        nf = (self.info()["ctus"] - at) // per if nframes is None else int(nframes)
        nf = max(nf, 0)
        sizes = {"codes": nf * per * SIM_CODE_BYTES, "reach": nf * per * 16}
        if planes:
            sizes["planes"] = nf * (height // 16) * (width // 16)
        bufs = {k: self.ctx.alloc(max(v, 16)) for k, v in sizes.items()}
        try:
            self.decide_frames_device(thr, gates, mid_k, at, width, height, nf, bufs["codes"], bufs["reach"], bufs.get("planes"))
            out = {k: bufs[k].download(np.uint8, v) if v else np.zeros(0, np.uint8) for k, v in sizes.items()}
        finally:
            for b in bufs.values():
                b.free()
        out["codes"], out["reach"] = out["codes"].reshape(-1, SIM_CODE_BYTES), out["reach"].reshape(-1, 16)
        if planes:
            out["planes"] = out["planes"].reshape(nf, height // 16, width // 16)
        return out

    # --------------------------------------------------------------------------------------------------------- search budget ---
    def _budget_window(self, ladder, width, height, first, nframes):
        """-> (ladder records, K, first CTU, frames): nframes None = to the end of the set"""
        ladder = budget_default_ladder(self.lib) if ladder is None else _sim_cands(ladder)
        width, height = int(width), int(height)
        if width <= 0 or height <= 0:
            raise ValueError("got %d x %d" % (width, height))
        nf = (self.info()["ctus"] - int(first)) // ctus_per_frame(width, height) if nframes is None else int(nframes)
        return ladder, ladder.size, int(first), max(nf, 0)

    def budget_cost(self, ladder=None, first=0, width=0, height=0, nframes=None):
        """the checks that every rung of `ladder` (SIM_THR records, default: budget_default_ladder()) leaves on each of nframes whole
        width x height frames from CTU `first` on (include/ethcnn.h "search budget") -> uint32 [F, K + 1, 4]: checked[0..3] per frame and
        rung, column K the full search"""
        ladder, k, first, nf = self._budget_window(ladder, width, height, first, nframes)
        out = np.zeros((nf, k + 1, 4), np.uint32)
        self._chk(self.lib.ethcnn_budget_cost(self.h, ladder.ctypes.data, k, first, int(width), int(height), nf, out.ctypes.data if nf else None))
        return out

    def budget_cost_device(self, ladder, first, width, height, nframes, d_checked):
        """the same into a buffer in HBM (DeviceBuffer or raw device address): [nframes, K + 1, 4] uint32"""
        ladder = budget_default_ladder(self.lib) if ladder is None else _sim_cands(ladder)
        self._chk(self.lib.ethcnn_budget_cost_device(self.h, ladder.ctypes.data, ladder.size, int(first), int(width), int(height), int(nframes),
                                                     getattr(d_checked, "ptr", d_checked)))

    def budget_bake(self, ladder, rung, first=0, width=0, height=0, nframes=None):
        """the decisions of rung[f] of `ladder` (None: the default ladder) on frame f, as the values an unchanged encoder reads under the
        companion thresholds -> float32 [n, 21]: 1.0 split only or frame edge, 0.0 current only or not visited, 0.5 both (a rejected
        CTU: 0.5 everywhere)"""
        ladder, k, first, nf = self._budget_window(ladder, width, height, first, nframes)
        rung = np.ascontiguousarray(rung, dtype=np.int32).reshape(-1)
        if rung.size != nf:
            raise ValueError("%d frames, %d rungs" % (nf, rung.size))
        out = np.zeros((nf * ctus_per_frame(int(width), int(height)), NOUT), np.float32)
        self._chk(self.lib.ethcnn_budget_bake(self.h, ladder.ctypes.data, k, rung.ctypes.data if nf else None, first, int(width), int(height), nf,
                                              out.ctypes.data if nf else None))
        return out

    def budget_bake_device(self, ladder, rung, first, width, height, nframes, d_probs):
        """the same into a buffer in HBM (DeviceBuffer or raw device address): [nframes * nctu, 21] float32; rung stays a host array"""
        ladder = budget_default_ladder(self.lib) if ladder is None else _sim_cands(ladder)
        rung = np.ascontiguousarray(rung, dtype=np.int32).reshape(-1)
        if rung.size != int(nframes):
            raise ValueError("%d frames, %d rungs" % (int(nframes), rung.size))
        self._chk(self.lib.ethcnn_budget_bake_device(self.h, ladder.ctypes.data, ladder.size, rung.ctypes.data if rung.size else None, int(first), int(width),
                                                     int(height), int(nframes), getattr(d_probs, "ptr", d_probs)))

    def budget_control(self, budget, mode="frame", ladder=None, weights=None, first=0, width=0, height=0, nframes=None, probs=True):
        """cost, choice and bake in one call.  budget: the share of the full search a frame may take, 0..1 (rounded to parts per
        million); mode "frame" (every frame on its own) or "carry" (what a frame leaves goes to the next) -> dict: probs float32 [n, 21]
        (unless probs=False), rung int32 [F], over bool [F], cost uint64 [F], full uint64 [F]"""
        if not 0.0 <= float(budget) <= 1.0:
            raise ValueError("the budget is a share of the full search, 0..1: got %r" % (budget,))
        lad, k, first, nf = self._budget_window(ladder, width, height, first, nframes)
        w = None if weights is None else (ctypes.c_uint64 * 4)(*[int(x) for x in weights])
        out = {"rung": np.zeros(nf, np.int32), "over": np.zeros(nf, np.uint8), "cost": np.zeros(nf, np.uint64), "full": np.zeros(nf, np.uint64)}
        if probs:
            out["probs"] = np.zeros((nf * ctus_per_frame(int(width), int(height)), NOUT), np.float32)
        ptr = lambda name: out[name].ctypes.data if name in out and out[name].size else None
        self._chk(self.lib.ethcnn_budget_control(self.h, None if ladder is None else lad.ctypes.data, k, w, int(round(float(budget) * 1e6)), _budget_mode(mode),
                                                 first, int(width), int(height), nf, ptr("probs"), ptr("rung"), ptr("over"), ptr("cost"), ptr("full")))
        out["over"] = out["over"].astype(bool)
        return out

    def build_ladder(self, weights=None, grid=8, max_rungs=4096, max_bad_ppm=10 ** 6):
        """a ladder for the search budget built from this set's labels (include/ethcnn.h "search budget: building a ladder"): a greedy
        walk from the full search, one threshold moved per rung, one launch per step -> dict of numpy arrays over the rungs: thr
        (SIM_THR records), coord int32 (-1 for rung 0), value int32, checked uint64 [n, 4], bad_ctus uint64, cost (Python integers)"""
        w = None if weights is None else (ctypes.c_uint64 * 4)(*[int(x) for x in weights])
        ladder_check(weights, grid, max_rungs, max_bad_ppm, self.lib)  # (sizes the output: a bad max_rungs never reaches np.zeros)
        rungs, n = np.zeros(int(max_rungs), LADDER_RUNG), ctypes.c_int64(0)
        self._chk(self.lib.ethcnn_ladder_build(self.h, w, int(grid), int(max_rungs), int(max_bad_ppm), rungs.ctypes.data, ctypes.byref(n)))
        rungs = rungs[:n.value]
        wt = [int(x) for x in (BUDGET_WEIGHTS if weights is None else weights)]
        cost = np.array([sum(a * int(b) for a, b in zip(wt, row)) for row in rungs["checked"]], dtype=object)
        return {"thr": np.ascontiguousarray(rungs["thr"]), "coord": rungs["coord"].copy(), "value": rungs["value"].copy(),
                "checked": rungs["checked"].copy(), "bad_ctus": rungs["bad_ctus"].copy(), "cost": cost}

    # ------------------------------------------------------------------------------------------- expected wrong decisions ---
    def set_reliability(self, rel=None):
        """the reliability table the expected wrong decisions are read from: uint32 [3, 1025] with values in 0..RISK_ONE (risk_from_hist,
        risk_read), or None for the identity table, which a simulator starts with"""
        if rel is not None:
            rel = _risk_table(rel)
        self._chk(self.lib.ethcnn_risk_set_reliability(self.h, None if rel is None else rel.ctypes.data))

    def eval_risk(self, cands):
        """the expected wrong_split[] / wrong_stop[] of every candidate under gates "none", from the probabilities alone (include/ethcnn.h
        "partition-search simulation: expected wrong decisions"): cands as for eval -> SIM_RISK records [K], in units of 1 / RISK_ONE"""
        cands = _sim_cands(cands)
        out = np.zeros(cands.size, SIM_RISK)
        self._chk(self.lib.ethcnn_risk_eval(self.h, cands.ctypes.data if cands.size else None, cands.size, out.ctypes.data if cands.size else None))
        return out

    def build_ladder_risk(self, weights=None, grid=8, max_rungs=4096, max_risk_ppm=2 ** 64 - 1):
        """build_ladder without labels: the same walk with the expected wrong decisions in place of the bad CTUs.  max_risk_ppm caps the
        expected wrong nodes per million counted CTUs (the default is no cap) -> dict of numpy arrays over the rungs: thr, coord, value,
        checked uint64 [n, 4], exp_wrong_split / exp_wrong_stop uint64 [n, 3], and risk and cost as Python integers"""
        w = None if weights is None else (ctypes.c_uint64 * 4)(*[int(x) for x in weights])
        ladder_check(weights, grid, max_rungs, 0, self.lib)  # (sizes the output: a bad max_rungs never reaches np.zeros)
        if not 0 <= int(max_risk_ppm) < 2 ** 64:
            raise EthCnnError(ERR_ARG, "max_risk_ppm lies in 0..2^64-1, got %r" % (max_risk_ppm,))
        rungs, n = np.zeros(int(max_rungs), LADDER_RUNG_RISK), ctypes.c_int64(0)
        self._chk(self.lib.ethcnn_risk_ladder_build(self.h, w, int(grid), int(max_rungs), int(max_risk_ppm), rungs.ctypes.data, ctypes.byref(n)))
        rungs = rungs[:n.value]
        wt = [int(x) for x in (BUDGET_WEIGHTS if weights is None else weights)]
        cost = np.array([sum(a * int(b) for a, b in zip(wt, row)) for row in rungs["checked"]], dtype=object)
        risk = np.array([sum(int(x) for x in a) + sum(int(x) for x in b) for a, b in zip(rungs["exp_wrong_split"], rungs["exp_wrong_stop"])], dtype=object)
        return {"thr": np.ascontiguousarray(rungs["thr"]), "coord": rungs["coord"].copy(), "value": rungs["value"].copy(), "checked": rungs["checked"].copy(),
                "exp_wrong_split": rungs["exp_wrong_split"].copy(), "exp_wrong_stop": rungs["exp_wrong_stop"].copy(), "risk": risk, "cost": cost}

    # ---------------------------------------------------------------------------- threshold calibration on reached nodes ---
    def reach_hist(self, cands, gates="none"):
        """the histogram of the decided nodes of the labelled CTUs under every candidate, in the calibrator's layout (include/ethcnn.h
        "threshold calibration on reached nodes"): cands as for eval, at most REACH_MAX_CAND -> uint64 [K, 3, 2, 1025] = [candidate, level,
        truth, bin].  calib_choose, risk_from_hist and write_thr_info take a candidate's histogram as they take Calibrator.histogram()"""
        cands = _sim_cands(cands)
        out = np.zeros((cands.size, CALIB_LEVELS, 2, CALIB_BINS), np.uint64)
        self._chk(self.lib.ethcnn_reach_hist(self.h, cands.ctypes.data if cands.size else None, cands.size, _SIM_GATES[gates],
                                             out.ctypes.data if cands.size else None))
        return out

    def calibrate_reached(self, eps_down_ppm, eps_up_ppm, gates="none"):
        """the six thresholds chosen top-down on the nodes the pruned search reaches: level l by calib_choose on the reach histogram under
        the levels above it.  Budgets in parts per million (three values, or one for all levels) -> (CalibReport, SIM_THR record,
        SIM_COUNTS record of that record under `gates`)"""
        rep, thr, counts = CalibReport(), np.zeros(1, SIM_THR), np.zeros(1, SIM_COUNTS)
        self._chk(self.lib.ethcnn_reach_calibrate(self.h, _ppm3(eps_down_ppm), _ppm3(eps_up_ppm), _SIM_GATES[gates], ctypes.byref(rep), thr.ctypes.data,
                                                  counts.ctypes.data))
        return rep, thr[0], counts[0]


# search budget: building a ladder (include/ethcnn.h).  ethcnn_ladder_rung as a numpy record: 72 bytes, no padding
LADDER_RUNG = np.dtype([("thr", SIM_THR), ("coord", "<i4"), ("value", "<i4"), ("checked", "<u8", (4,)), ("bad_ctus", "<u8")])

# expected wrong decisions (include/ethcnn.h "partition-search simulation: expected wrong decisions"): the unit, ethcnn_sim_risk and
# ethcnn_ladder_rung_risk (112 bytes, no padding) as numpy records
RISK_ONE = 1 << 20
RISK_BINS = 1025
SIM_RISK = np.dtype([("exp_wrong_split", "<u8", (3,)), ("exp_wrong_stop", "<u8", (3,))])
LADDER_RUNG_RISK = np.dtype([("thr", SIM_THR), ("coord", "<i4"), ("value", "<i4"), ("checked", "<u8", (4,)), ("exp_wrong_split", "<u8", (3,)),
                             ("exp_wrong_stop", "<u8", (3,))])


def _risk_table(rel):
    """a reliability table as contiguous uint32 [3, 1025]; ValueError for another shape or a value that uint32 cannot hold"""
    a = np.asarray(rel)
    if a.size != 3 * RISK_BINS or (a.size and (a.min() < 0 or a.max() >= 2 ** 32)):
        raise ValueError("a reliability table is [3, %d] integers in 0..%d" % (RISK_BINS, RISK_ONE))
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(3, RISK_BINS)


def risk_identity(lib=None):
    """ethcnn_risk_identity (host only): the table rel[l][b] = b * 1024 that takes the model at its word -> uint32 [3, 1025]"""
    lib = lib or load_library()
    rel = np.zeros((3, RISK_BINS), np.uint32)
    rc = lib.ethcnn_risk_identity(rel.ctypes.data)
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return rel


def risk_from_hist(hist, lib=None):
    """ethcnn_risk_from_hist (host only): the non-decreasing table fitted to a calibrator's histogram uint64 [3, 2, 1025]
    (Calibrator.histogram) by pool-adjacent-violators -> uint32 [3, 1025]"""
    lib = lib or load_library()
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    if hist.size != 3 * 2 * RISK_BINS:
        raise ValueError("the histogram is [3, 2, %d], got %d words" % (RISK_BINS, hist.size))
    rel = np.zeros((3, RISK_BINS), np.uint32)
    rc = lib.ethcnn_risk_from_hist(hist.ctypes.data, rel.ctypes.data)
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return rel


def risk_write(path, rel, lib=None):
    """ethcnn_risk_write (host only): the table as a text file (temp file + rename)"""
    lib = lib or load_library()
    rel = _risk_table(rel)
    rc = lib.ethcnn_risk_write(os.fsencode(path), rel.ctypes.data)
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())


def risk_read(path, lib=None):
    """ethcnn_risk_read (host only): a table file -> uint32 [3, 1025]; EthCnnError (ERR_FORMAT, ERR_IO) names what is wrong with it"""
    lib = lib or load_library()
    rel = np.zeros((3, RISK_BINS), np.uint32)
    rc = lib.ethcnn_risk_read(os.fsencode(path), rel.ctypes.data)
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return rel


def _int_arg(x, lo, hi):
    """an integer argument of a C entry, clamped into [lo, hi] so that ctypes takes it; the library names a value outside its rules"""
    return max(lo, min(hi, int(x)))


def ladder_check(weights=None, grid=8, max_rungs=4096, max_bad_ppm=10 ** 6, lib=None):
    """ethcnn_ladder_check (host only): the argument rules of PartitionSim.build_ladder; EthCnnError where the library says ETHCNN_ERR_ARG"""
    lib = lib or load_library()
    w = None
    if weights is not None:
        if len(weights) != 4 or min(int(x) for x in weights) < 0:
            raise ValueError("weights are four non-negative integers W64 W32 W16 W8, got %r" % (weights,))
        w = (ctypes.c_uint64 * 4)(*[min(int(x), 2 ** 64 - 1) for x in weights])
    rc = lib.ethcnn_ladder_check(w, _int_arg(grid, -1, 2 ** 31 - 1), _int_arg(max_rungs, -1, 2 ** 63 - 1), _int_arg(max_bad_ppm, 0, 2 ** 32 - 1))
    if rc or int(max_bad_ppm) < 0:
        raise EthCnnError(rc or ERR_ARG, lib.ethcnn_last_error(None).decode() if rc else "max_bad_ppm is negative")


def ladder_thin(cost, K, lib=None):
    """ethcnn_ladder_thin (host only): the indices of at most K of the rungs whose costs (strictly falling integers below 2^64) are
    given, evenly spaced in cost; rungs 0 and n - 1 are always kept -> int32 array"""
    lib = lib or load_library()
    cost = [int(x) for x in cost]
    if cost and (min(cost) < 0 or max(cost) >= 2 ** 64):
        raise ValueError("costs lie in 0..2^64-1")
    c = np.array(cost, dtype=np.uint64)
    idx, k = np.zeros(max(1, min(len(cost), max(int(K), 1))), np.int32), ctypes.c_int64(0)
    rc = lib.ethcnn_ladder_thin(c.ctypes.data if c.size else None, c.size, _int_arg(K, -1, 2 ** 63 - 1), idx.ctypes.data, ctypes.byref(k))
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())
    return idx[:k.value]


def ladder_write(path, thr, order, lib=None):
    """ethcnn_ladder_write (host only): SIM_THR records as a ladder file, one rung per line in the token order "ai" or "ldp" -- what
    tools/control_budget.py --ladder and ETHCNN_SEARCH_BUDGET_LADDER read"""
    lib = lib or load_library()
    if order not in _THR_ORDERS:
        raise ValueError("order is 'ai' or 'ldp', got %r" % (order,))
    thr = _sim_cands(thr)
    rc = lib.ethcnn_ladder_write(os.fsencode(path), thr.ctypes.data if thr.size else None, thr.size, _THR_ORDERS[order])
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())


# search budget, online (include/ethcnn.h "search budget, online")
# ethcnn_pacer_result as a numpy record: 72 bytes, no padding
PACER_RESULT = np.dtype([("frame", "<i8"), ("rung", "<i4"), ("over", "<i4"), ("cost", "<u8"), ("full", "<u8"), ("carry_lo", "<u8"), ("carry_hi", "<u8"),
                         ("up_k", "<i4", (3,)), ("down_k", "<i4", (3,))])


def _budget_ppm(budget):
    if not 0.0 <= float(budget) <= 1.0:
        raise ValueError("the budget is a share of the full search, 0..1: got %r" % (budget,))
    return int(round(float(budget) * 1e6))


def pacer_check(budget_ppm, mode=BUDGET_FRAME, ladder=None, weights=None, lib=None):
    """ethcnn_pacer_check (host only): the argument rules of a pacer -- ladder (SIM_THR records, None: the default), weights (None: 64 16
    4 1), budget in parts per million, mode as a number; EthCnnError where the library says ETHCNN_ERR_ARG"""
    lib = lib or load_library()
    lad = None if ladder is None else _sim_cands(ladder)
    w = None if weights is None else (ctypes.c_uint64 * 4)(*[int(x) for x in weights])
    rc = lib.ethcnn_pacer_check(None if lad is None else lad.ctypes.data, 0 if lad is None else lad.size, w, int(budget_ppm), int(mode))
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())


class Pacer(object):
    """The search budget held one frame at a time (include/ethcnn.h "search budget, online"): owns the ladder, the weights, the budget
    (a share 0..1), the mode ("frame" or "carry"), the carry and the frame count; a frame is two launches on the context's stream."""

    def __init__(self, ctx, budget, mode="frame", ladder=None, weights=None):
        self.ctx, self.lib = ctx, ctx.lib
        lad = None if ladder is None else _sim_cands(ladder)
        w = None if weights is None else (ctypes.c_uint64 * 4)(*[int(x) for x in weights])
        h = ctypes.c_void_p()
        ctx._chk(self.lib.ethcnn_pacer_create(ctx.h, None if lad is None else lad.ctypes.data, 0 if lad is None else lad.size, w, _budget_ppm(budget),
                                              _budget_mode(mode), ctypes.byref(h)))
        self.h = h
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)  # closed with the context, before it

    def _chk(self, rc):
        self.ctx._chk(rc)

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the pacer is closed")
        return self.h

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_pacer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        """carry = 0, frame = 0 (in stream order behind the frames already queued)"""
        self._chk(self.lib.ethcnn_pacer_reset(self._handle()))

    def frame(self, probs, width, height, out=None):
        """one frame: probs float32 [nctu, 21] (a host array; a view of ctx.host_buffer() is used in place) -> (baked float32 [nctu, 21],
        result record).  out: the array the baked rows go to (None: a new one; `probs` itself: in place)"""
        n = ctus_per_frame(int(width), int(height))
        probs = np.ascontiguousarray(probs, dtype=np.float32)
        if probs.size != n * NOUT:
            raise ValueError("a %d x %d frame has %d x 21 probabilities, got %d values" % (width, height, n, probs.size))
        baked = np.empty((n, NOUT), np.float32) if out is None else out
        assert baked.dtype == np.float32 and baked.size == n * NOUT and baked.flags["C_CONTIGUOUS"]
        res = np.zeros(1, PACER_RESULT)
        self._chk(self.lib.ethcnn_pacer_frame(self._handle(), probs.ctypes.data, int(width), int(height), baked.ctypes.data, res.ctypes.data))
        return baked.reshape(n, NOUT), res[0]

    def frame_device(self, d_probs, width, height, d_baked, d_result=None):
        """the same on buffers in HBM (DeviceBuffer or raw device addresses), asynchronous on the context's stream; d_baked may be
        d_probs; d_result (72 bytes) may be None"""
        ptr = lambda b: None if b is None else getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_pacer_frame_device(self._handle(), ptr(d_probs), int(width), int(height), ptr(d_baked), ptr(d_result)))

    def last(self):
        """the result record of the most recent frame (synchronous)"""
        res = np.zeros(1, PACER_RESULT)
        self._chk(self.lib.ethcnn_pacer_last(self._handle(), res.ctypes.data))
        return res[0]


# search budget, online: several sequences (include/ethcnn.h)
PACER_SET_MAX = 32


class PacerSetFrame(ctypes.Structure):
    """ethcnn_pacer_set_frame"""
    _fields_ = [("slot", ctypes.c_int), ("probs", ctypes.c_void_p), ("width", ctypes.c_int), ("height", ctypes.c_int), ("baked", ctypes.c_void_p),
                ("result", ctypes.c_void_p)]


PACER_SET_MAX_POLICIES = 32


class PacerPolicy(ctypes.Structure):
    """ethcnn_pacer_policy"""
    _fields_ = [("ladder", ctypes.c_void_p), ("K", ctypes.c_int64), ("weight", ctypes.c_void_p), ("budget_ppm", ctypes.c_uint32), ("mode", ctypes.c_int32)]


def _pacer_policies(policies, ppm=_budget_ppm, mode=_budget_mode):
    """dicts {budget, mode, ladder, weights} (mode "frame", ladder None and weights None by default) -> (a C array of ethcnn_pacer_policy,
    the arrays its pointers point into); ppm and mode turn a dict's budget and mode into the numbers of the C struct"""
    arr = (PacerPolicy * max(len(policies), 1))()
    keep = []
    for i, q in enumerate(policies[:len(arr)]):
        extra = set(q) - {"budget", "mode", "ladder", "weights"}
        if extra:
            raise ValueError("policy %d: unknown keys %s" % (i, sorted(extra)))
        lad = None if q.get("ladder") is None else _sim_cands(q["ladder"])
        w = None if q.get("weights") is None else (ctypes.c_uint64 * 4)(*[int(x) for x in q["weights"]])
        keep += [lad, w]
        arr[i] = PacerPolicy(None if lad is None else lad.ctypes.data, 0 if lad is None else lad.size, None if w is None else ctypes.addressof(w),
                             ppm(q["budget"]), mode(q.get("mode", "frame")))
    return arr, keep


def _slot_policy(slot_policy):
    return None if slot_policy is None else (ctypes.c_int * max(len(slot_policy), 1))(*[int(x) for x in slot_policy])


def pacer_set_check_policies(policies, slot_policy=None, raw=False, lib=None):
    """ethcnn_pacer_policies_check (host only): the rules of a PacerSet's policies -- dicts {budget (a share 0..1), mode, ladder,
    weights} -- and of slot_policy, a policy index per slot (None: none to check); EthCnnError with the policy index in the message
    where the library says ETHCNN_ERR_ARG.  raw: budget is in parts per million and mode a number, both passed on as they are"""
    lib = lib or load_library()
    arr, keep = _pacer_policies(policies, int, int) if raw else _pacer_policies(policies)
    sp = _slot_policy(slot_policy)
    rc = lib.ethcnn_pacer_policies_check(arr if len(policies) else None, len(policies), sp, 0 if slot_policy is None else len(slot_policy))
    if rc:
        raise EthCnnError(rc, lib.ethcnn_last_error(None).decode())


def pacer_set_plan(nctus, K=512, lib=None):
    """ethcnn_pacer_set_plan (host only): the layout of a PacerSet call over frames of these CTU counts, in this order, under K + 1 rungs
    -> {"count_first", "count_blocks", "slice_len", "bake_first", "rec0": one entry per frame, "count_grid", "bake_grid"}; EthCnnError
    for bad arguments.  K may be a list, one entry per frame (ethcnn_pacer_policies_plan): frame j under K[j] + 1 rungs, those of the
    policy its slot is bound to"""
    lib = lib or load_library()
    n = len(nctus)
    counts = np.array([min(max(int(x), -1), 2 ** 62) for x in nctus], np.int64)
    out = {k: np.zeros(max(n, 1), np.int32 if k == "slice_len" else np.int64) for k in ("count_first", "count_blocks", "slice_len", "bake_first", "rec0")}
    grids = np.zeros(2, np.int64)
    if isinstance(K, (list, tuple, np.ndarray)):
        if len(K) != n:
            raise ValueError("%d frames and %d entries of K" % (n, len(K)))
        each = np.array([_int_arg(x, -1, 2 ** 63 - 1) for x in K], np.int64)
        rc = lib.ethcnn_pacer_policies_plan(counts.ctypes.data if n else None, each.ctypes.data if n else None, n, out["count_first"].ctypes.data,
                                             out["count_blocks"].ctypes.data, out["slice_len"].ctypes.data, out["bake_first"].ctypes.data,
                                             out["rec0"].ctypes.data, grids.ctypes.data, grids.ctypes.data + 8)
    else:
        rc = lib.ethcnn_pacer_set_plan(counts.ctypes.data if n else None, n, _int_arg(K, -1, 2 ** 63 - 1), out["count_first"].ctypes.data,
                                       out["count_blocks"].ctypes.data, out["slice_len"].ctypes.data, out["bake_first"].ctypes.data, out["rec0"].ctypes.data,
                                       grids.ctypes.data, grids.ctypes.data + 8)
    if rc:
        raise EthCnnError(rc, "ethcnn_pacer_set_plan: bad arguments")
    res = {k: [int(x) for x in v[:n]] for k, v in out.items()}
    res.update(count_grid=int(grids[0]), bake_grid=int(grids[1]))
    return res


class PacerSet(object):
    """Up to 32 paced sequences behind one ladder, one weight vector, one budget (a share 0..1) and one mode (include/ethcnn.h "search
    budget, online: several sequences"): a slot owns the carry, the frame count and the result of one sequence, a call paces any subset
    of the slots by one frame each in two launches on the context's stream.  Slot by slot the results and the baked rows are a Pacer's.
    PacerSet(ctx, nslots, policies=[{budget, mode, ladder, weights}, ...], slot_policy=None) holds up to 32 policies instead of one:
    slot s is bound to policies[slot_policy[s]] (None: all to the first) until bind(s, policy), and is a Pacer of that policy."""

    def __init__(self, ctx, nslots, budget=None, mode="frame", ladder=None, weights=None, policies=None, slot_policy=None):
        self.ctx, self.lib = ctx, ctx.lib
        h = ctypes.c_void_p()
        if policies is not None:
            if budget is not None or ladder is not None or weights is not None or mode != "frame":
                raise ValueError("a PacerSet takes either one budget, mode, ladder and weights or a list of policies")
            if slot_policy is not None and len(slot_policy) != int(nslots):
                raise ValueError("slot_policy has %d entries for %d slots" % (len(slot_policy), int(nslots)))
            arr, keep = _pacer_policies(list(policies))
            ctx._chk(self.lib.ethcnn_pacer_policies_create(ctx.h, int(nslots), arr if len(policies) else None, len(policies), _slot_policy(slot_policy),
                                                               ctypes.byref(h)))
        else:
            if budget is None:
                raise TypeError("a PacerSet needs a budget or a list of policies")
            if slot_policy is not None:
                raise ValueError("slot_policy belongs to a list of policies")
            lad = None if ladder is None else _sim_cands(ladder)
            w = None if weights is None else (ctypes.c_uint64 * 4)(*[int(x) for x in weights])
            ctx._chk(self.lib.ethcnn_pacer_set_create(ctx.h, int(nslots), None if lad is None else lad.ctypes.data, 0 if lad is None else lad.size, w,
                                                      _budget_ppm(budget), _budget_mode(mode), ctypes.byref(h)))
        self.h = h
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)  # closed with the context, before it

    def _chk(self, rc):
        self.ctx._chk(rc)

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the pacer set is closed")
        return self.h

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_pacer_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __len__(self):
        return max(0, int(self.lib.ethcnn_pacer_set_slots(self._handle())))

    @property
    def launches(self):
        """kernels the set has enqueued since it was made"""
        return int(self.lib.ethcnn_pacer_set_launches(self._handle()))

    def reset(self, slot):
        """carry = 0, frame = 0 of that slot (in stream order behind the frames already queued)"""
        self._chk(self.lib.ethcnn_pacer_set_reset(self._handle(), int(slot)))

    @property
    def npolicies(self):
        return max(0, int(self.lib.ethcnn_pacer_policies_count(self._handle())))

    def policy_of(self, slot):
        """the index of the policy that slot is bound to"""
        rc = int(self.lib.ethcnn_pacer_policies_of(self._handle(), int(slot)))
        if rc < 0:
            self._chk(rc)
        return rc

    def bind(self, slot, policy):
        """reset(slot), and from the next call on that slot is paced under policies[policy] (in stream order behind the frames already
        queued, which keep the policy they were queued under); binding to the policy the slot has is a reset"""
        self._chk(self.lib.ethcnn_pacer_policies_bind(self._handle(), int(slot), int(policy)))

    def frames_device(self, frames):
        """asynchronous on the context's stream (ethcnn_pacer_set_frames_device).  frames: one dict per frame with slot, d_probs, width,
        height, d_baked (DeviceBuffers or raw device addresses; d_baked may be d_probs) and optionally d_result (72 bytes, None)"""
        ptr = lambda b: None if b is None else getattr(b, "ptr", b)
        arr = (PacerSetFrame * max(len(frames), 1))()
        for j, f in enumerate(frames[:len(arr)]):
            arr[j] = PacerSetFrame(int(f["slot"]), ptr(f["d_probs"]), int(f["width"]), int(f["height"]), ptr(f["d_baked"]), ptr(f.get("d_result")))
        self._chk(self.lib.ethcnn_pacer_set_frames_device(self._handle(), arr, len(frames)))

    def frames(self, frames):
        """synchronous, host memory (ethcnn_pacer_set_frames).  frames: one dict per frame with slot, probs (float32 [nctu, 21]; a view of
        ctx.host_buffer() is used in place), width, height and optionally out (the array the baked rows go to; None: a new one; the
        `probs` array itself: in place) -> (the baked arrays [nctu, 21], the result records), both in call order"""
        arr = (PacerSetFrame * max(len(frames), 1))()
        res = np.zeros(max(len(frames), 1), PACER_RESULT)
        keep, outs = [], []
        for j, f in enumerate(frames[:len(arr)]):
            n = ctus_per_frame(int(f["width"]), int(f["height"]))
            probs = np.ascontiguousarray(f["probs"], dtype=np.float32)
            if probs.size != n * NOUT:
                raise ValueError("frame %d: a %d x %d frame has %d x 21 probabilities, got %d values" % (j, f["width"], f["height"], n, probs.size))
            out = f.get("out")
            if out is None:
                out = np.empty((n, NOUT), np.float32)
            elif out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"] or out.size != n * NOUT:
                raise ValueError("frame %d: out must be a contiguous float32 array of %d values" % (j, n * NOUT))
            keep.append(probs)
            outs.append(out)
            arr[j] = PacerSetFrame(int(f["slot"]), probs.ctypes.data, int(f["width"]), int(f["height"]), out.ctypes.data, res.ctypes.data + j * PACER_RESULT.itemsize)
        self._chk(self.lib.ethcnn_pacer_set_frames(self._handle(), arr, len(frames)))
        return [o.reshape(-1, NOUT) for o in outs], [res[j] for j in range(len(frames))]

    def last(self, slot):
        """the result record of that slot's most recent frame (synchronous)"""
        res = np.zeros(1, PACER_RESULT)
        self._chk(self.lib.ethcnn_pacer_set_last(self._handle(), int(slot), res.ctypes.data))
        return res[0]


# ------------------------------------------------------------------------------------- config #5 offline, group form ---
def _ptr_array(bufs):
    """DeviceBuffers / raw device addresses / None -> a C array of pointers"""
    vals = [None if b is None else getattr(b, "ptr", b) for b in bufs]
    return (ctypes.c_void_p * max(len(vals), 1))(*vals)


class _LdpSet(object):
    """what LdpGroup and LdpBatch share: the handle behind ethcnn_<_PREFIX>_*, its bundles (i: a group's member, a batch's bundle
    index) and its resident states (j: a group's member, a batch's sequence index)"""
    _PREFIX = None  # "ldp_group" or "ldp_batch"

    def _fn(self, name):
        return getattr(self.lib, "ethcnn_%s_%s" % (self._PREFIX, name))

    def _gates_fn(self, verb):
        """ethcnn_ldp_sessions_<verb>_thresholds; for a group and a batch the form comes last: ethcnn_ldp_<verb>_thresholds_group"""
        form = self._PREFIX[4:]
        return getattr(self.lib, "ethcnn_ldp_sessions_%s_thresholds" % verb if form == "sessions" else "ethcnn_ldp_%s_thresholds_%s" % (verb, form))

    def __init__(self, ctx, count):
        self.ctx, self.lib = ctx, ctx.lib
        h = ctypes.c_void_p()
        ctx._chk(self._fn("create")(ctx.h, int(count), ctypes.byref(h)))
        self.h = h
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)  # closed with the context, before it

    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self._fn("last_error")(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_lstm_checkpoint(self, i, prefix):
        self._chk(self._fn("load_lstm_checkpoint")(self.h, int(i), os.fsencode(prefix)))

    def load_lstm_blob(self, i, blob):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        self._chk(self._fn("load_lstm_blob")(self.h, int(i), blob.ctypes.data_as(_fp), blob.size))

    def load_lstm_synthetic(self, i, seed=1, head_gain=1.0):
        self._chk(self._fn("load_lstm_synthetic")(self.h, int(i), int(seed), float(head_gain)))

    def get_lstm_blob(self, i):
        out = np.empty(LSTM_BLOB_FLOATS, dtype=np.float32)
        self._chk(self._fn("get_lstm_blob")(self.h, int(i), out.ctypes.data_as(_fp), out.size))
        return out

    def _set_chunk(self, frames):
        self._chk(self._fn("set_chunk")(self.h, int(frames)))

    def state_ctus(self, j):
        """the CTU count of the resident state of member / sequence index j (0: none)"""
        n = int(self._fn("state_ctus")(self.h, int(j)))
        self._chk(n if n < 0 else 0)
        return n

    def get_state(self, j):
        """the resident (c, h) state of member / sequence index j -> float32 [nctu, 2, 448]"""
        state = np.empty((self.state_ctus(j), 2, NVEC), dtype=np.float32)
        self._chk(self._fn("get_state")(self.h, int(j), state.ctypes.data_as(_fp), state.size))
        return state

    def set_thresholds(self, j, thr_l1_lower, thr_l2_lower):
        """a gate pair of its own for member / sequence index / session j: from now on j runs under it, whatever the context's is"""
        self._chk(self._gates_fn("set")(self.h, int(j), thr_l1_lower, thr_l2_lower))

    def clear_thresholds(self, j):
        """j inherits the context's pair again (as it stands when a call is made)"""
        self._chk(self._gates_fn("clear")(self.h, int(j)))

    def thresholds_of(self, j):
        """-> (thr_l1_lower, thr_l2_lower, own): the pair j runs under now; own = 0: it is the context's"""
        a, b, own = ctypes.c_float(), ctypes.c_float(), ctypes.c_int()
        self._chk(self._gates_fn("get")(self.h, int(j), ctypes.byref(a), ctypes.byref(b), ctypes.byref(own)))
        return a.value, b.value, own.value


class LdpGroup(_LdpSet):
    """K = 1..8 Low-Delay-P residual sequences of one geometry through one recurrence launch (include/ethcnn.h "config #5 offline,
    group form"): each member has its own ETH-LSTM bundle, QP, resident state and output, and its result equals
    EthCnn.ldp_sequence_device on a context that holds its bundle, bit for bit.  The residual CNN is the context's, and so are the
    thresholds of every member that has no pair of its own (set_thresholds); the context's own LSTM bundle and resident state are
    not touched."""
    _PREFIX = "ldp_group"

    def __init__(self, ctx, k):
        _LdpSet.__init__(self, ctx, k)

    def __len__(self):
        return max(0, int(self.lib.ethcnn_ldp_group_count(self.h)))

    set_chunk_frames = _LdpSet._set_chunk

    def sequence_device(self, d_lumas, width, height, nframes, qps, i_frame_first, d_probs, d_state_ins=None, pitch=None, frame_stride=None):
        """asynchronous on the context's stream (ethcnn_ldp_group_sequence_device): one luma buffer, QP and probability buffer per
        member (DeviceBuffers or raw device addresses); d_state_ins: None, or one entry per member of which any may be None"""
        k = len(self)
        if len(d_lumas) != k or len(qps) != k or len(d_probs) != k or (d_state_ins is not None and len(d_state_ins) != k):
            raise ValueError("sequence_device takes one entry per member (%d)" % k)
        pitch = width if pitch is None else pitch
        frame_stride = pitch * height if frame_stride is None else frame_stride
        self._chk(self.lib.ethcnn_ldp_group_sequence_device(self.h, _ptr_array(d_lumas), width, height, pitch, frame_stride, int(nframes),
                                                            (ctypes.c_int * k)(*[int(q) for q in qps]), int(i_frame_first),
                                                            None if d_state_ins is None else _ptr_array(d_state_ins), _ptr_array(d_probs)))

    def sequence(self, lumas, width, height, qps, i_frame_first=1, state_ins=None):
        """lumas: one uint8 array [nframes, height, width] per member, in host memory -> a list of probs [nframes, nctu, 21].  The
        inputs are uploaded to DeviceBuffers and the results downloaded (a convenience for small inputs: a job keeps its frames in HBM
        and calls sequence_device).  state_ins: None, or per member None / float32 [nctu, 2, 448]."""
        k, n = len(self), ctus_per_frame(width, height)
        lumas = [np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, height, width) for a in lumas]
        if len(lumas) != k or len(set(a.shape[0] for a in lumas)) != 1:
            raise ValueError("sequence takes %d inputs of one frame count" % k)
        nframes = lumas[0].shape[0]
        bufs = []
        alloc = lambda nbytes: bufs.append(DeviceBuffer(self.ctx, max(int(nbytes), 4))) or bufs[-1]
        try:
            d_l, d_p, d_s = [], [], None
            for a in lumas:
                d_l.append(alloc(a.nbytes))
                d_l[-1].upload(a)
                d_p.append(alloc(nframes * n * NOUT * 4))
            if state_ins is not None:
                d_s = []
                for st in state_ins:
                    d_s.append(None)
                    if st is not None:
                        d_s[-1] = alloc(n * 2 * NVEC * 4)
                        d_s[-1].upload(np.ascontiguousarray(st, dtype=np.float32).reshape(n, 2, NVEC))
            self.sequence_device(d_l, width, height, nframes, qps, i_frame_first, d_p, d_s)
            return [b.download(np.float32, nframes * n * NOUT).reshape(nframes, n, NOUT) for b in d_p]
        finally:
            self.ctx.synchronize()
            for b in bufs:
                b.free()


# ------------------------------------------------------------------------------------- config #5 offline, batch form ---
class LdpBatchSeq(ctypes.Structure):
    """ethcnn_ldp_batch_seq"""
    _fields_ = [("d_luma", ctypes.c_void_p), ("width", ctypes.c_int), ("height", ctypes.c_int), ("pitch", ctypes.c_ssize_t),
                ("frame_stride", ctypes.c_ssize_t), ("nframes", ctypes.c_int), ("qp", ctypes.c_int), ("i_frame_first", ctypes.c_int),
                ("bundle", ctypes.c_int), ("d_state_in", ctypes.c_void_p), ("d_probs", ctypes.c_void_p)]


class LdpBatch(_LdpSet):
    """Up to 32 Low-Delay-P residual sequences of different geometry, length and first frame number through one recurrence launch
    per chunk (include/ethcnn.h "config #5 offline, batch form").  The object holds nbundles = 1..8 ETH-LSTM bundles; a sequence names
    its bundle by index, and its result equals EthCnn.ldp_sequence_device on a context that holds that bundle, bit for bit.  The
    residual CNN is the context's, and so are the thresholds of every sequence index that has no pair of its own (set_thresholds);
    the context's own LSTM bundle and resident state are not touched."""
    _PREFIX = "ldp_batch"

    def __init__(self, ctx, nbundles):
        _LdpSet.__init__(self, ctx, nbundles)

    @property
    def nbundles(self):
        return max(0, int(self.lib.ethcnn_ldp_batch_bundles(self.h)))

    set_chunk = _LdpSet._set_chunk

    def run_device(self, seqs):
        """asynchronous on the context's stream (ethcnn_ldp_batch_run_device).  seqs: one dict per sequence with d_luma, width, height,
        nframes, qp, d_probs (DeviceBuffers or raw device addresses) and optionally i_frame_first (1), bundle (0), d_state_in (None),
        pitch (width), frame_stride (pitch * height)"""
        ptr = lambda b: None if b is None else getattr(b, "ptr", b)
        arr = (LdpBatchSeq * max(len(seqs), 1))()
        for j, q in enumerate(seqs[:len(arr)]):
            pitch = int(q.get("pitch") or q["width"])
            arr[j] = LdpBatchSeq(ptr(q["d_luma"]), int(q["width"]), int(q["height"]), pitch, int(q.get("frame_stride") or pitch * int(q["height"])),
                                 int(q["nframes"]), int(q["qp"]), int(q.get("i_frame_first", 1)), int(q.get("bundle", 0)), ptr(q.get("d_state_in")),
                                 ptr(q["d_probs"]))
        self._chk(self.lib.ethcnn_ldp_batch_run_device(self.h, arr, len(seqs)))

    def run(self, seqs):
        """seqs: one dict per sequence with luma (uint8 [nframes, height, width], host memory), width, height, qp and optionally
        i_frame_first, bundle, state_in (float32 [nctu, 2, 448]) -> a list of probs [nframes, nctu, 21].  The inputs are uploaded to
        DeviceBuffers and the results downloaded (a convenience for small inputs: a job keeps its frames in HBM and calls run_device)."""
        bufs, dev, shapes = [], [], []
        alloc = lambda nbytes: bufs.append(DeviceBuffer(self.ctx, max(int(nbytes), 4))) or bufs[-1]
        try:
            for q in seqs:
                w, h = int(q["width"]), int(q["height"])
                n = ctus_per_frame(w, h)
                luma = np.ascontiguousarray(q["luma"], dtype=np.uint8).reshape(-1, h, w)
                d = {k: q[k] for k in ("width", "height", "qp", "i_frame_first", "bundle") if k in q}
                d["nframes"] = luma.shape[0]
                d["d_luma"] = alloc(luma.nbytes)
                d["d_luma"].upload(luma)
                d["d_probs"] = alloc(luma.shape[0] * n * NOUT * 4)
                if q.get("state_in") is not None:
                    d["d_state_in"] = alloc(n * 2 * NVEC * 4)
                    d["d_state_in"].upload(np.ascontiguousarray(q["state_in"], dtype=np.float32).reshape(n, 2, NVEC))
                dev.append(d)
                shapes.append((luma.shape[0], n))
            self.run_device(dev)
            return [d["d_probs"].download(np.float32, nf * n * NOUT).reshape(nf, n, NOUT) for d, (nf, n) in zip(dev, shapes)]
        finally:
            self.ctx.synchronize()
            for b in bufs:
                b.free()


# ------------------------------------------------------------------------------- config #5 online, several live encoders ---
class LdpSessionFrame(ctypes.Structure):
    """ethcnn_ldp_session_frame"""
    _fields_ = [("session", ctypes.c_int), ("luma", ctypes.c_void_p), ("pitch", ctypes.c_ssize_t), ("qp", ctypes.c_int), ("i_frame", ctypes.c_int),
                ("bundle", ctypes.c_int), ("state_in", ctypes.c_void_p), ("probs", ctypes.c_void_p)]


class LdpSessions(_LdpSet):
    """Up to 32 live Low-Delay-P encoders on one context (include/ethcnn.h "config #5 online, several live encoders"): a session has a
    picture size and a resident recurrent state, a step advances any subset of the sessions by one frame through one shared front-end
    and one recurrence launch.  The object holds nbundles = 1..8 ETH-LSTM bundles; a frame names its bundle by index, and its result
    equals EthCnn.ldp_step on a context of its own that holds that bundle, bit for bit.  The residual CNN is the context's, and so
    are the thresholds of every session that has no pair of its own (set_thresholds; close forgets it); the context's own LSTM bundle
    and resident state are not touched."""
    _PREFIX = "ldp_sessions"

    def __init__(self, ctx, nbundles):
        _LdpSet.__init__(self, ctx, nbundles)
        self._size = {}  # session id -> (width, height)

    @property
    def nbundles(self):
        return max(0, int(self.lib.ethcnn_ldp_sessions_bundles(self.h)))

    def open(self, width, height):
        """-> the id of a new session for width x height pictures (ids are reused after close)"""
        sid = ctypes.c_int(-1)
        self._chk(self.lib.ethcnn_ldp_sessions_open(self.h, int(width), int(height), ctypes.byref(sid)))
        self._size[sid.value] = (int(width), int(height))
        return sid.value

    def close_session(self, session):
        self._chk(self.lib.ethcnn_ldp_sessions_close(self.h, int(session)))
        self._size.pop(int(session), None)

    def close(self, session=None):
        """close(session): forget that session; close(): destroy the object (as the other handles' close does)"""
        if session is None:
            _LdpSet.close(self)
        else:
            self.close_session(session)

    def step_device(self, frames):
        """asynchronous on the context's stream (ethcnn_ldp_sessions_step_device).  frames: one dict per frame with session, d_luma, qp,
        i_frame, d_probs (DeviceBuffers or raw device addresses) and optionally bundle (0), d_state_in (None), pitch (the width)"""
        ptr = lambda b: None if b is None else getattr(b, "ptr", b)
        arr = (LdpSessionFrame * max(len(frames), 1))()
        for j, f in enumerate(frames[:len(arr)]):
            pitch = f.get("pitch") or self._size.get(int(f["session"]), (0, 0))[0]
            arr[j] = LdpSessionFrame(int(f["session"]), ptr(f["d_luma"]), int(pitch), int(f["qp"]), int(f["i_frame"]), int(f.get("bundle", 0)),
                                     ptr(f.get("d_state_in")), ptr(f["d_probs"]))
        self._chk(self.lib.ethcnn_ldp_sessions_step_device(self.h, arr, len(frames)))

    def step(self, frames):
        """synchronous, host memory (ethcnn_ldp_sessions_step).  frames: one dict per frame with session, luma (uint8 [height, width], or
        [height, pitch] with pitch given), qp, i_frame and optionally bundle (0), state_in (float32 [nctu, 2, 448]), probs_out (a
        float32 array of nctu x 21 to write into) -> a list of probs [nctu, 21]"""
        arr = (LdpSessionFrame * max(len(frames), 1))()
        keep, outs = [], []
        for j, f in enumerate(frames[:len(arr)]):
            w, h = self._size.get(int(f["session"]), (0, 0))
            n = ctus_per_frame(w, h) if w else 0
            luma = np.ascontiguousarray(f["luma"], dtype=np.uint8)
            pitch = int(f.get("pitch") or w)
            if w and luma.size < (h - 1) * pitch + w:
                raise ValueError("frame %d: the luma buffer is smaller than a %dx%d picture at pitch %d" % (j, w, h, pitch))
            sin = f.get("state_in")
            if sin is not None:
                sin = np.ascontiguousarray(sin, dtype=np.float32)
                if sin.size != n * 2 * NVEC:
                    raise ValueError("frame %d: state_in must hold %d floats" % (j, n * 2 * NVEC))
            out = f.get("probs_out")
            if out is None:
                out = np.empty((n, NOUT), dtype=np.float32)
            elif out.dtype != np.float32 or not out.flags["C_CONTIGUOUS"] or out.size != n * NOUT:
                raise ValueError("frame %d: probs_out must be a contiguous float32 array of %d values" % (j, n * NOUT))
            keep.append((luma, sin))
            outs.append(out)
            arr[j] = LdpSessionFrame(int(f["session"]), luma.ctypes.data, pitch, int(f["qp"]), int(f["i_frame"]), int(f.get("bundle", 0)),
                                     None if sin is None else sin.ctypes.data, out.ctypes.data)
        self._chk(self.lib.ethcnn_ldp_sessions_step(self.h, arr, len(frames)))
        return [o.reshape(-1, NOUT) for o in outs]


# ------------------------------------------------------------------------------------------------------ sample-set replay ---
class ReplayRun(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32),
                ("f0", ctypes.c_uint32), ("frames", ctypes.c_int64), ("nctu", ctypes.c_int64), ("qp", ctypes.c_int32 * 4),
                ("src_offset", ctypes.c_int64)]

    def as_dict(self):
        return {"seq": self.seq, "w": self.w, "h": self.h, "rows": self.rows, "cols": self.cols, "f0": self.f0, "frames": self.frames,
                "nctu": self.nctu, "qps": [int(q) for q in self.qp]}


def _record_bytes(x):
    """bytes / uint8 array / path of a file of 16516-byte records -> a contiguous uint8 array (a file is mapped, not read)"""
    if isinstance(x, (str, os.PathLike)):
        return np.memmap(x, dtype=np.uint8, mode="r") if os.path.getsize(x) else np.empty(0, np.uint8)
    return np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, np.uint8).reshape(-1)


def replay_plan(records, lib=None):
    """ethcnn_replay_plan on uint8 LDP records (host only, any record order): a list of runs, each the dict of ReplayRun.as_dict plus
    "src", int64 [frames, nctu]: the index of the record at (f0 + frame, line, col), CTUs in raster order.  Raises EthCnnError
    (ERR_FORMAT) with the record and the rule for an invalid file."""
    lib = lib or load_library()
    buf = _record_bytes(records)
    n = buf.size // LDP_RECORD_BYTES
    src, nruns, err = np.empty(max(n, 1), np.int64), ctypes.c_int(0), ctypes.create_string_buffer(800)
    rc = lib.ethcnn_replay_plan(buf.ctypes.data if buf.size else None, buf.size, None, 0, ctypes.byref(nruns), src.ctypes.data, err, 800)
    runs = (ReplayRun * max(nruns.value, 1))()
    if not rc:
        rc = lib.ethcnn_replay_plan(buf.ctypes.data, buf.size, ctypes.byref(runs), nruns.value, ctypes.byref(nruns), None, err, 800)
    if rc:
        raise EthCnnError(rc, err.value.decode("utf-8", "replace") or "ethcnn_replay_plan: bad arguments")
    out = []
    for r in runs[:nruns.value]:
        d = r.as_dict()
        d["src"] = src[r.src_offset: r.src_offset + r.frames * r.nctu].reshape(r.frames, r.nctu).copy()
        out.append(d)
    return out


def replay_uncut_device(ctx, d_records, nrecords, d_src, nframes, rows, cols, slot, d_resi, d_labels):
    """ethcnn_replay_uncut_device: the uncut kernel on buffers in HBM (DeviceBuffers or raw device addresses); asynchronous"""
    ptr = lambda b: getattr(b, "ptr", b)
    ctx._chk(ctx.lib.ethcnn_replay_uncut_device(ctx.h, ptr(d_records), int(nrecords), ptr(d_src), int(nframes), int(rows), int(cols), int(slot),
                                                ptr(d_resi), ptr(d_labels)))


class Replay(object):
    """An inter sample set run through the deployed Low-Delay-P chain (include/ethcnn.h "sample-set replay"): the residual pictures and
    label planes of every sequence the set holds are put back together in HBM, in any record order, and go through ldp_sequence as the
    daemon would run them.  max_bytes: the most device memory a replay may hold (0 = no limit of its own)."""

    def __init__(self, ctx, max_bytes=0):
        self.ctx, self.lib, self.max_bytes = ctx, ctx.lib, int(max_bytes)
        h = ctypes.c_void_p()
        ctx._chk(self.lib.ethcnn_replay_create(ctx.h, int(max_bytes), ctypes.byref(h)))
        self.h = h
        self._source = None  # a SampleSet that is open stays alive with this object
        if not hasattr(ctx, "_trainers"):
            ctx._trainers = weakref.WeakSet()
        ctx._trainers.add(self)  # closed with the context, before it

    def _chk(self, rc):
        if rc:
            raise EthCnnError(rc, self.lib.ethcnn_replay_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ethcnn_replay_destroy(self.h)
            self.h = None
        self._source = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def open(self, x):
        """x: a built inter SampleSet (read in HBM, left as it is), a uint8 array / bytes of 16516-byte records, or the path of a file
        of them.  Replaces whatever was open."""
        self._source = None
        if isinstance(x, SampleSet):
            self._chk(self.lib.ethcnn_replay_open_set(self.h, x.h))
            self._source = x
            return self
        buf = _record_bytes(x)
        self._chk(self.lib.ethcnn_replay_open_records(self.h, buf.ctypes.data if buf.size else None, buf.size))
        return self

    def set_chunk_frames(self, frames):
        self._chk(self.lib.ethcnn_replay_set_chunk_frames(self.h, int(frames)))

    def __len__(self):
        return max(0, int(self.lib.ethcnn_replay_run_count(self.h)))

    def run_info(self, i):
        r = ReplayRun()
        self._chk(self.lib.ethcnn_replay_run_info(self.h, int(i), ctypes.byref(r)))
        return r.as_dict()

    def runs(self):
        return [self.run_info(i) for i in range(len(self))]

    def slot_of(self, i, qp):
        """the slot of run i whose QP byte is qp (ValueError when there is none)"""
        qps = self.run_info(i)["qps"]
        if int(qp) not in qps:
            raise ValueError("QP %d is not one of the slot QPs %s of run %d" % (qp, qps, i))
        return qps.index(int(qp))

    def run_bytes(self, i, own_probs=False, own_labels=False):
        """device bytes run_device holds for run i (own_*: without a buffer of the caller's)"""
        n = int(self.lib.ethcnn_replay_run_bytes(self.h, int(i), int(bool(own_probs)), int(bool(own_labels))))
        self._chk(n if n < 0 else 0)
        return n

    def run_device(self, i, slot, d_probs=None, d_labels=None):
        """asynchronous on the context's stream: probabilities float32 [frames, nctu, 21] and labels uint8 [frames, 4 rows, 4 cols] of run
        i at QP slot `slot` into buffers in HBM (DeviceBuffers or raw addresses; None: the object's own)"""
        ptr = lambda b: None if b is None else getattr(b, "ptr", b)
        self._chk(self.lib.ethcnn_replay_run_device(self.h, int(i), int(slot), ptr(d_probs), ptr(d_labels)))

    def run(self, i, slot):
        """-> (probs float32 [frames, nctu, 21], labels uint8 [frames, 4 rows, 4 cols]) in host memory"""
        r = self.run_info(i)
        n = r["frames"] * r["nctu"]
        dp, dl = DeviceBuffer(self.ctx, n * NOUT * 4), DeviceBuffer(self.ctx, n * 16)
        try:
            self.run_device(i, slot, dp, dl)
            probs = dp.download(np.float32, n * NOUT).reshape(r["frames"], r["nctu"], NOUT)
            labels = dl.download(np.uint8, n * 16).reshape(r["frames"], 4 * r["rows"], 4 * r["cols"])
        finally:
            self.ctx.synchronize()
            dp.free()
            dl.free()
        return probs, labels

    def run_group_bytes(self, i, nslots):
        """device bytes run_group_device holds for run i with nslots slots replayed together (the group's own memory apart)"""
        n = int(self.lib.ethcnn_replay_run_group_bytes(self.h, int(i), int(nslots)))
        self._chk(n if n < 0 else 0)
        return n

    def run_group_device(self, i, slots, group, d_probs, d_labels):
        """asynchronous on the context's stream: run i at every listed QP slot through an LdpGroup (member j takes slots[j] with that
        slot's QP and the bundle loaded into member j); d_probs[j] float32 [frames, nctu, 21] and d_labels[j] uint8 [frames, 4 rows,
        4 cols] in HBM (DeviceBuffers or raw addresses), one each per slot"""
        slots = [int(x) for x in slots]
        if len(d_probs) != len(slots) or len(d_labels) != len(slots):
            raise ValueError("run_group_device takes one probability and one label buffer per slot")
        self._chk(self.lib.ethcnn_replay_run_group_device(self.h, int(i), len(slots), (ctypes.c_int * max(len(slots), 1))(*slots), group.h,
                                                          _ptr_array(d_probs), _ptr_array(d_labels)))

    def run_group(self, i, slots, group):
        """-> [(probs float32 [frames, nctu, 21], labels uint8 [frames, 4 rows, 4 cols])] in host memory, one pair per listed slot"""
        r = self.run_info(i)
        n = r["frames"] * r["nctu"]
        bufs = []
        try:
            for _ in slots:
                bufs.append((DeviceBuffer(self.ctx, n * NOUT * 4), DeviceBuffer(self.ctx, n * 16)))
            self.run_group_device(i, slots, group, [b[0] for b in bufs], [b[1] for b in bufs])
            return [(dp.download(np.float32, n * NOUT).reshape(r["frames"], r["nctu"], NOUT),
                     dl.download(np.uint8, n * 16).reshape(r["frames"], 4 * r["rows"], 4 * r["cols"])) for dp, dl in bufs]
        finally:
            self.ctx.synchronize()
            for dp, dl in bufs:
                dp.free()
                dl.free()

    def run_batch_bytes(self, runs, batch):
        """device bytes run_batch_device holds for these runs replayed together (the batch's own memory apart)"""
        n = int(self.lib.ethcnn_replay_batch_bytes(self.h, batch.h, len(runs), _int_array(runs)))
        self._chk(n if n < 0 else 0)
        return n

    def run_batch_device(self, items, batch, d_probs, d_labels):
        """asynchronous on the context's stream: items = [(run, slot, bundle)], up to 32, through an LdpBatch in one recurrence launch
        per chunk; d_probs[j] float32 [frames, nctu, 21] and d_labels[j] uint8 [frames, 4 rows, 4 cols] of item j in HBM"""
        if len(d_probs) != len(items) or len(d_labels) != len(items):
            raise ValueError("run_batch_device takes one probability and one label buffer per item")
        self._chk(self.lib.ethcnn_replay_batch_device(self.h, batch.h, len(items), _int_array([it[0] for it in items]), _int_array([it[1] for it in items]),
                                                      _int_array([it[2] for it in items]), _ptr_array(d_probs), _ptr_array(d_labels)))

    def run_batch(self, items, batch):
        """items = [(run, slot, bundle)] -> [(probs float32 [frames, nctu, 21], labels uint8 [frames, 4 rows, 4 cols])] in host memory"""
        info = [self.run_info(it[0]) for it in items]
        bufs = []
        try:
            for r in info:
                n = r["frames"] * r["nctu"]
                bufs.append((DeviceBuffer(self.ctx, n * NOUT * 4), DeviceBuffer(self.ctx, n * 16)))
            self.run_batch_device(items, batch, [b[0] for b in bufs], [b[1] for b in bufs])
            return [(dp.download(np.float32, r["frames"] * r["nctu"] * NOUT).reshape(r["frames"], r["nctu"], NOUT),
                     dl.download(np.uint8, r["frames"] * r["nctu"] * 16).reshape(r["frames"], 4 * r["rows"], 4 * r["cols"]))
                    for r, (dp, dl) in zip(info, bufs)]
        finally:
            self.ctx.synchronize()
            for dp, dl in bufs:
                dp.free()
                dl.free()

    def _pack(self, runs, batch):
        """the runs, in order, in lists of at most 32 whose memory sum as a feed holds it (ethcnn_replay_batch_bytes and the object's own
        outputs, 100 bytes per CTU) stays within the object's limit; a run that exceeds it alone goes alone, and is refused with the
        sum by the call"""
        packs, cur = [], []
        own = lambda lst: sum(r["frames"] * r["nctu"] * (NOUT * 4 + 16) for r in (self.run_info(i) for i in lst))
        for i in runs:
            if cur and (len(cur) == LDP_BATCH_MAX or (self.max_bytes and self.run_batch_bytes(cur + [i], batch) + own(cur + [i]) > self.max_bytes)):
                packs.append(cur)
                cur = []
            cur.append(int(i))
        return packs + ([cur] if cur else [])

    def feed(self, consumer, runs=None, slot=None, qp=None, batch=None, bundle_of=None):
        """replays the listed runs (None: all) at `slot`, or at the slot of each run that holds `qp`, into a Calibrator or a
        PartitionSim without leaving HBM.  The context's gates should be open (set_thresholds(0, 0)), as for any input of those two.
        batch: an LdpBatch; the runs are then packed in order into batches of at most 32 that stay within max_bytes and go through one
        recurrence launch per chunk each, with bundle bundle_of(run, slot) of the batch (None: bundle 0) in place of the context's;
        the consumer ends in the state the per-run feeds leave."""
        if (slot is None) == (qp is None):
            raise ValueError("feed takes slot= or qp=")
        if isinstance(consumer, Calibrator):
            fn, bfn = self.lib.ethcnn_replay_feed_calib, self.lib.ethcnn_replay_batch_feed_calib
        elif isinstance(consumer, PartitionSim):
            fn, bfn = self.lib.ethcnn_replay_feed_sim, self.lib.ethcnn_replay_batch_feed_sim
        else:
            raise TypeError("feed takes a Calibrator or a PartitionSim")
        runs = list(range(len(self)) if runs is None else runs)
        slot_for = lambda i: int(slot) if slot is not None else self.slot_of(i, qp)
        if batch is None:
            for i in runs:
                self._chk(fn(self.h, int(i), slot_for(i), consumer.h))
            return
        for pack in self._pack(runs, batch):
            slots = [slot_for(i) for i in pack]
            bundles = [0 if bundle_of is None else int(bundle_of(i, s)) for i, s in zip(pack, slots)]
            self._chk(bfn(self.h, batch.h, len(pack), _int_array(pack), _int_array(slots), _int_array(bundles), consumer.h))
