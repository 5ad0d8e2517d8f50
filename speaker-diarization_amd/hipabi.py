"""ctypes binding of include/spkd.h (libspkd_hip.so).  No torch here: device
memory is addressed by raw pointers (``tensor.data_ptr()`` or ``dev_alloc``)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (SPKD_HIP_LIBRARY: another build of the same library, for A/B measurements)
LIB_PATH = os.environ.get('SPKD_HIP_LIBRARY') or os.path.join(HERE, 'csrc', 'libspkd_hip.so')

SPKD_OK, SPKD_EINVAL, SPKD_EHIP, SPKD_ENONFINITE, SPKD_EOVERFLOW, SPKD_ENOMEM = range(6)
# 'KL2P': KL2 with the reference's pseudo-inverse (SPKD_KL2_PINV); 'KL2' is the inverse
KINDS = {'BIC': 0, 'GLR': 1, 'KL2': 2, 'KL2P': 3}
WANT_GLR, WANT_KL2, WANT_KL2_PINV = 1, 2, 4
MERGE_NO_AHEAD = 1
TIMERS = {n: i for i, n in enumerate(['call', 'chunk_stats', 'reduce_sets', 'pair_terms',
                                        'cluster_prep', 'matrix', 'ahc', 'gw', 'sw', 'merge',
                                        'vad_shift', 'vad_viterbi', 'vad_backtrack', 'gauss_models', 'gauss_loglik',
                                        'post_stats', 'bf_gcc', 'bf_track', 'bf_sum', 'resample', 'frame_energy', 'energy_seeds',
                                        'feature_warp', 'tdoa_pack', 'tdoa_stats', 'tdoa_models', 'tdoa_score', 'tdoa_cuts', 'tdoa_split', 'tdoa_second', 'tdoa_overlap', 'gmm_train', 'gmm_seq_loglik', 'ubm_stats', 'clr_link',
                                        'mindur_viterbi', 'mindur_backtrack', 'fb_posterior',
                                        'ident_scores', 'ident_assign', 'bw_accumulate',
                                        'mfcc_static', 'mfcc_post'])}
VAD_TILE = 32       # SPKD_VAD_TILE: frames per score / back-pointer tile of k_vad_viterbi
MINDUR_TILE = 32    # SPKD_MINDUR_TILE: frames per score / record tile of k_mindur_viterbi
FB_TILE = 32        # SPKD_FB_TILE: frames per score tile and per stored forward vector of k_fb_posterior
POST_CHUNK = 1024   # SPKD_POST_CHUNK: frames per workgroup of k_post_chunk_stats
GAUSS_TILE = 64     # SPKD_GAUSS_TILE: frames per workgroup of k_gauss_loglik
GAUSS_MODEL = 820   # SPKD_GAUSS_MODEL: doubles per model (mu[39], W = L^-1 packed lower [780], c)
GMM_COMP = 80       # SPKD_GMM_COMP: doubles per mixture component (ln w, mean[39], 1 / var[39], log_norm)
GMM_MAX_COMP = 8    # SPKD_GMM_MAX_COMP: components per speaker
GMM_TILE = 64       # SPKD_GMM_TILE: frame ordinals per tile of k_gmm_estep, frames per workgroup of k_gmm_loglik_seq
GMM_CHUNK_TILES = 16    # SPKD_GMM_CHUNK_TILES: tiles per chunk, the unit of a partial sum of k_gmm_estep
BW_COMP = 40        # SPKD_BW_COMP: doubles per component of a speaker record under a UBM (n_c, f_c[39])
CLR_MAX_N = 4096    # SPKD_CLR_MAX_N: speakers of one spkd_clr_link
GALLERY_MAX_N = 16384   # SPKD_GALLERY_MAX_N: identities of one spkd_clr_identify
MFCC_POST_TILE = 128    # SPKD_MFCC_POST_TILE: frames per workgroup of k_mfcc_post
MFCC_POST_HALO = 4      # SPKD_MFCC_POST_HALO: frames to either side of a tile whose first deltas it forms
MFCC_POST_LDS = 61440   # SPKD_MFCC_POST_LDS: bytes of LDS a tile of k_mfcc_post may take
MFCC_CMS_MAX = 272      # SPKD_MFCC_CMS_MAX: the widest mean window, cms_left + cms_right, that fits them
RESAMPLE_TILE = 2048        # SPKD_RESAMPLE_TILE: output samples per workgroup of k_resample
RESAMPLE_MAX_CH = 8         # SPKD_RESAMPLE_MAX_CH: channels of a file
RESAMPLE_MAX_HALF = 256     # SPKD_RESAMPLE_MAX_HALF: taps to either side of an output instant
RESAMPLE_MAX_TERM = 1 << 20     # SPKD_RESAMPLE_MAX_TERM: up and down of a conversion
RESAMPLE_MAX_TAPS = 1 << 22     # SPKD_RESAMPLE_MAX_TAPS: floats of one conversion's table
RESAMPLE_MAX_SPAN = 33281   # SPKD_RESAMPLE_MAX_SPAN: input frames a tile may read
BF_NFFT = 8192              # SPKD_BF_NFFT: the transform length of k_bf_gcc; window + max_lag of a geometry fit it
BF_NBEST = 4                # SPKD_BF_NBEST: candidate lags kept per step and channel
BF_MAX_HOP = 1 << 20        # SPKD_BF_MAX_HOP: the largest hop of a geometry
ENERGY_MAX_WINDOW = 4096    # SPKD_ENERGY_MAX_WINDOW: samples of a frame of k_frame_energy (hop <= window)
ENERGY_TILE = 16384         # SPKD_ENERGY_TILE: samples whose hops make the frames of a workgroup of k_frame_energy
TDOA_NONE = -(1 << 31)      # SPKD_TDOA_NONE: a step of the delay stream that is not reliable on a channel
TDOA_MAX_CH = 8             # SPKD_TDOA_MAX_CH: channels of a file of the delay stream
TDOA_MAX_DELAY = 4096       # SPKD_TDOA_MAX_DELAY: the largest |delay| of an entry
TDOA_FILE = 8               # SPKD_TDOA_FILE: int64 per file of the stream's host table
TDOA_MODEL = 4              # SPKD_TDOA_MODEL: doubles per (speaker, channel): mean, var, 1 / (2 var), -1/2 log(2 pi var)
TDOA_TILE = 256             # SPKD_TDOA_TILE: frames per workgroup of k_tdoa_score, steps per workgroup of k_tdoa_stats
SEAT_MAX_N = 4096           # SPKD_SEAT_MAX_N: records of one problem of spkd_tdoa_split
OVERLAP_MAX_SPK = 16        # SPKD_OVERLAP_MAX_SPK: speakers of a file of spkd_tdoa_overlap
OVERLAP_MAX_RUN = 64        # SPKD_OVERLAP_MAX_RUN: the largest min_steps of spkd_tdoa_overlap
WARP_MAX_WINDOW = 512       # SPKD_WARP_MAX_WINDOW: the widest window of spkd_feature_warp, in frames
WARP_TILE = 384             # SPKD_WARP_TILE: compacted frames per workgroup of k_feature_warp
REC = 820
DIM = 39

EXPORTS = ['spkd_abi_version', 'spkd_create', 'spkd_create_on_stream', 'spkd_destroy', 'spkd_last_error', 'spkd_sync',
           'spkd_malloc', 'spkd_free', 'spkd_memcpy_h2d', 'spkd_memcpy_d2h', 'spkd_memcpy_d2d',
           'spkd_last_kernel_ms', 'spkd_last_gw_items', 'spkd_last_ahc_head', 'spkd_ahc_head_rule', 'spkd_set_stats', 'spkd_pair_terms',
           'spkd_distance_matrix', 'spkd_gw_event_capacity', 'spkd_gw_event_capacity_p', 'spkd_gw', 'spkd_gw_ex', 'spkd_gw_fused', 'spkd_gw_batch', 'spkd_ahc_fused', 'spkd_gather_stats', 'spkd_sum_stats', 'spkd_mfcc', 'spkd_mfcc_batch', 'spkd_resample_batch', 'spkd_bf_gcc', 'spkd_bf_track', 'spkd_bf_sum',
           'spkd_tdoa_pack', 'spkd_tdoa_stats', 'spkd_tdoa_models', 'spkd_tdoa_score', 'spkd_tdoa_cuts', 'spkd_tdoa_split', 'spkd_tdoa_second', 'spkd_tdoa_overlap',
           'spkd_sw_window_count', 'spkd_sw', 'spkd_sw_runs', 'spkd_sw_batch', 'spkd_merge_batch', 'spkd_ahc', 'spkd_ahc_matrix', 'spkd_distance_rows', 'spkd_cluster_in', 'spkd_cluster_in_batch', 'spkd_py2_roundtrip',
           'spkd_labels_from_merges', 'spkd_labels_from_merges_batch', 'spkd_count_flags', 'spkd_gw_lines',
           'spkd_gmm_loglik', 'spkd_vad_viterbi', 'spkd_vad_shift_batch', 'spkd_vad_viterbi_batch',
           'spkd_gauss_models', 'spkd_gauss_loglik', 'spkd_gmm_train', 'spkd_gmm_loglik_seq',
           'spkd_ubm_stats', 'spkd_clr_link', 'spkd_feature_warp', 'spkd_mindur_viterbi_batch', 'spkd_fb_posterior_batch',
           'spkd_clr_identify', 'spkd_bw_accumulate', 'spkd_post_stats', 'spkd_frame_energy_batch', 'spkd_energy_seeds']


class CdParams(C.Structure):
    _fields_ = [('kind', C.c_int32), ('trace', C.c_int32), ('lambdac', C.c_double),
                ('threshold', C.c_double), ('winsize', C.c_double), ('winstep', C.c_double),
                ('deltaws', C.c_double), ('rate', C.c_double)]


class CandLog(C.Structure):
    _fields_ = [('turn', C.c_int32), ('coarse', C.c_int32), ('seq', C.c_int64),
                ('start', C.c_double), ('i', C.c_double), ('d', C.c_double),
                ('n1', C.c_int64), ('n2', C.c_int64)]


class GwLinesView(C.Structure):
    _fields_ = [('n_lines', C.c_int64), ('n_redo', C.c_int64), ('n_win', C.c_void_p), ('times', C.c_void_p),
                ('turn', C.c_void_p), ('frame_b', C.c_void_p), ('frame_e', C.c_void_p), ('index', C.c_void_p),
                ('d_index', C.c_void_p), ('redo_line', C.c_void_p), ('redo_begin', C.c_void_p),
                ('redo_end', C.c_void_p)]


AHC_AUTO, AHC_MONO, AHC_WIDE = 0, 1, 2


class MfccParams(C.Structure):
    _fields_ = [('sample_rate', C.c_int32), ('frame_rate', C.c_int32), ('window_width', C.c_int32),
                ('n_fft', C.c_int32), ('n_mel', C.c_int32), ('n_cep', C.c_int32), ('cms_left', C.c_int32),
                ('cms_right', C.c_int32), ('delta_width', C.c_int32 * 2), ('pre_emph', C.c_float),
                ('delta_norm', C.c_float * 2)]


class ResampleConv(C.Structure):
    """spkd_resample_conv: up / down of a conversion, the taps to either side of an output instant
    and where its table [up][2 half_taps] starts in the concatenated tables."""
    _fields_ = [('up', C.c_int32), ('down', C.c_int32), ('half_taps', C.c_int32), ('taps_off', C.c_int64)]


class BfGeom(C.Structure):
    """spkd_bf_geom: hop, window and largest lag of a beamforming geometry, in samples."""
    _fields_ = [('hop', C.c_int32), ('window', C.c_int32), ('max_lag', C.c_int32)]


class GmmParams(C.Structure):
    _fields_ = [('n_kernels', C.c_int32), ('n_states', C.c_int32), ('dim', C.c_int32), ('mean', C.c_void_p),
                ('inv_var', C.c_void_p), ('log_norm', C.c_void_p), ('state_off', C.c_void_p), ('kernel', C.c_void_p),
                ('log_weight', C.c_void_p)]


class AhcParams(C.Structure):
    _fields_ = [('variant', C.c_int32), ('kind', C.c_int32), ('max_spk', C.c_int32),
                ('path', C.c_int32), ('lambdac', C.c_double), ('threshold', C.c_double)]


class SpkdError(RuntimeError):
    def __init__(self, status, text):
        RuntimeError.__init__(self, 'spkd status %d: %s' % (status, text))
        self.status = status


_lib = None


def _one_hip_runtime():
    """A process must hold ONE HIP runtime.  PyTorch wheels bundle their own
    (torch/lib/libamdhip64.so): if this library is loaded first it pulls in the system
    runtime, and a later `import torch` finds that foreign runtime under its soname and
    reports "No HIP GPUs are available".  So when a PyTorch installation is present but not
    imported yet, its runtime is loaded first (the wheel's file only: torch itself is not
    imported), and libspkd_hip.so binds to it -- the same situation as after `import
    torch`.  SPKD_SYSTEM_HIP=1 keeps the system runtime."""
    import sys
    if 'torch' in sys.modules or os.environ.get('SPKD_SYSTEM_HIP'):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
        where = list(spec.submodule_search_locations)[0] if spec and spec.submodule_search_locations else None
    except (ImportError, ValueError, AttributeError):
        where = None
    if where:
        rt = os.path.join(where, 'lib', 'libamdhip64.so')
        if os.path.exists(rt):
            try:
                C.CDLL(rt, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def mapped_hip_runtimes():
    """The distinct libamdhip64 files mapped into this process (from /proc/self/maps)."""
    found = set()
    try:
        with open('/proc/self/maps') as f:
            for line in f:
                path = line.rsplit(None, 1)[-1] if '/' in line else ''
                if os.path.basename(path).startswith('libamdhip64.so'):
                    found.add(os.path.realpath(path))
    except OSError:
        pass
    return sorted(found)


def _check_one_runtime():
    """After libspkd_hip.so is loaded exactly one HIP runtime must be mapped: the preload of
    the PyTorch wheel's runtime only helps when its soname is the one this library was linked
    against -- otherwise the loader brings in the system runtime as well, silently, which is
    the very situation the preload is meant to prevent.  Two runtimes: an error
    naming both, and the way out (SPKD_SYSTEM_HIP=1 for torch-free processes; importing torch
    before this package otherwise)."""
    rts = mapped_hip_runtimes()
    if len(rts) > 1:
        raise ImportError('two HIP runtimes are mapped into this process (%s): libspkd_hip.so and the PyTorch '
                          'wheel link against different libamdhip64 sonames.  Set SPKD_SYSTEM_HIP=1 for a '
                          'torch-free process, or import torch before this package.' % ', '.join(rts))


def load_library(path=None):
    """Loads libspkd_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError('HIP extension %s is not built: run `python -c "import __graft_entry__ as g; '
                          'g.build()"` (or make -C speaker-diarization_amd/csrc)' % p)
    _one_hip_runtime()
    lib = C.CDLL(p)
    _check_one_runtime()
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_double
    P = C.POINTER
    lib.spkd_abi_version.restype = C.c_int
    lib.spkd_create.argtypes = [C.c_int, vp, P(vp)]
    lib.spkd_create_on_stream.argtypes = [C.c_int, vp, P(vp)]
    lib.spkd_destroy.argtypes = [vp]
    lib.spkd_destroy.restype = None
    lib.spkd_last_error.argtypes = [vp]
    lib.spkd_last_error.restype = C.c_char_p
    lib.spkd_sync.argtypes = [vp]
    lib.spkd_malloc.argtypes = [vp, C.c_size_t, P(vp)]
    lib.spkd_free.argtypes = [vp, vp]
    lib.spkd_memcpy_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    lib.spkd_memcpy_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    lib.spkd_memcpy_d2d.argtypes = [vp, vp, vp, C.c_size_t]
    lib.spkd_last_kernel_ms.argtypes = [vp, C.c_int, P(C.c_float)]
    lib.spkd_last_gw_items.argtypes = [vp, P(C.c_int64)]
    lib.spkd_last_ahc_head.argtypes = [vp, P(C.c_int64)]
    lib.spkd_ahc_head_rule.argtypes = [vp, i64]
    lib.spkd_ahc_head_rule.restype = i64
    lib.spkd_set_stats.argtypes = [vp, vp, i64, vp, vp, vp, i64, i64, vp]
    lib.spkd_pair_terms.argtypes = [vp, vp, vp, vp, i64, C.c_int, vp]
    lib.spkd_distance_matrix.argtypes = [vp, C.c_int, dbl, vp, i64, vp]
    lib.spkd_gw_event_capacity.argtypes = [i64, dbl]
    lib.spkd_gw_event_capacity.restype = i64
    lib.spkd_gw_event_capacity_p.argtypes = [i64, P(CdParams)]
    lib.spkd_gw_event_capacity_p.restype = i64
    lib.spkd_gw.argtypes = [vp, vp, i64, vp, vp, i64, P(CdParams), vp, vp, vp, vp, vp, vp, vp, vp,
                            vp, i64, P(i64)]
    lib.spkd_gw_ex.argtypes = [vp, vp, i64, vp, vp, i64, P(CdParams), vp, C.c_int, vp, vp, vp, vp, vp, vp,
                               vp, vp, i64, P(i64)]
    lib.spkd_gw_fused.argtypes = [vp, vp, i64, vp, vp, i64, P(CdParams), vp, C.c_int, vp, vp, vp, vp, vp, vp,
                                  vp, vp, vp, i64, P(i64)]
    lib.spkd_gw_batch.argtypes = [vp, vp, i64, vp, vp, i64, P(CdParams), vp, vp, vp, vp, vp, vp, C.c_int, P(GwLinesView)]
    lib.spkd_ahc_fused.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, vp, i64, P(AhcParams),
                                   P(vp), P(vp), P(vp), P(vp), P(vp)]
    lib.spkd_gather_stats.argtypes = [vp, vp, i64, vp, vp, i64, i64, vp]
    lib.spkd_sum_stats.argtypes = [vp, vp, i64, vp, vp, i64, vp]
    lib.spkd_mfcc.argtypes = [vp, vp, i64, P(MfccParams), vp, vp, vp, vp, vp, vp, P(i64)]
    lib.spkd_mfcc_batch.argtypes = [vp, vp, i64, vp, P(MfccParams), vp, vp, vp, vp, vp, vp, vp]
    lib.spkd_resample_batch.argtypes = [vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.spkd_bf_gcc.argtypes = [vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.spkd_bf_track.argtypes = [vp, i64, vp, vp, vp, vp, i32, C.c_float, dbl, i32, vp]
    lib.spkd_bf_sum.argtypes = [vp, vp, i64, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.spkd_tdoa_pack.argtypes = [vp, vp, vp, C.c_float, i64, vp]
    lib.spkd_tdoa_stats.argtypes = [vp, vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, vp, i64, i64, vp]
    lib.spkd_tdoa_models.argtypes = [vp, vp, i64, vp, vp, vp, i64, i32, dbl, vp, vp]
    lib.spkd_tdoa_score.argtypes = [vp, vp, i64, vp, i64, i32, i32, i32, vp, i64, vp, i64, vp, vp, vp, vp, vp, i32, dbl, vp]
    lib.spkd_tdoa_cuts.argtypes = [vp, vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, i64, i64, i32, dbl, dbl, dbl, vp, vp]
    lib.spkd_tdoa_split.argtypes = [vp, vp, i64, vp, vp, vp, i64, i32, i32, i32, i32, dbl, dbl, dbl, vp, vp, vp, vp, vp]
    lib.spkd_tdoa_second.argtypes = [vp, vp, vp, vp, i32, C.c_float, C.c_float, i32, i64, vp]
    lib.spkd_tdoa_overlap.argtypes = [vp, vp, i64, vp, i64, i32, i32, i32, vp, vp, vp, vp, dbl, i32, i32, vp]
    lib.spkd_frame_energy_batch.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp]
    lib.spkd_energy_seeds.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, P(vp), P(vp), P(vp)]
    lib.spkd_sw_window_count.argtypes = [i64, dbl, dbl]
    lib.spkd_sw_window_count.restype = i64
    lib.spkd_sw.argtypes = [vp, vp, i64, vp, vp, i64, P(CdParams), vp, vp]
    lib.spkd_sw_runs.argtypes = [vp, vp, vp, i64, P(CdParams), vp] + [vp] * 10
    lib.spkd_sw_batch.argtypes = [vp, vp, i64, vp, vp, i64, P(CdParams), vp, vp, i64] + [vp] * 11
    lib.spkd_merge_batch.argtypes = [vp, vp, i64, i64, vp, vp, vp, C.c_int, dbl, dbl, C.c_int] + [vp] * 9
    lib.spkd_ahc.argtypes = [vp, vp, vp, i64, P(AhcParams), vp, vp, vp, vp, vp, vp]
    lib.spkd_ahc_matrix.argtypes = [vp, vp, i64, P(AhcParams), vp, dbl, dbl, vp, vp, vp, vp, vp, vp]
    lib.spkd_distance_rows.argtypes = [vp, C.c_int, C.c_int, dbl, vp, i64, i64, i64, vp, P(dbl), P(dbl)]
    lib.spkd_cluster_in.argtypes = [vp, vp, i64, C.c_int, dbl, dbl, vp, vp, i64, vp, P(i64), P(i64)]
    lib.spkd_cluster_in_batch.argtypes = [vp, vp, i64, vp, C.c_int, dbl, dbl, vp, vp, vp, vp, vp, vp]
    lib.spkd_py2_roundtrip.argtypes = [vp, i64]
    lib.spkd_py2_roundtrip.restype = None
    lib.spkd_labels_from_merges.argtypes = [i64, i64, vp, vp, vp]
    lib.spkd_labels_from_merges_batch.argtypes = [i64, vp, vp, vp, vp, vp]
    lib.spkd_count_flags.argtypes = [vp, vp, vp, i64, vp]
    lib.spkd_gmm_loglik.argtypes = [vp, vp, i64, P(GmmParams), vp]
    lib.spkd_vad_viterbi.argtypes = [i64, i32, vp, i32, vp, vp, vp, vp, vp, vp, P(i64), P(dbl)]
    lib.spkd_vad_shift_batch.argtypes = [vp, vp, i64, vp, i32, dbl, vp]
    lib.spkd_vad_viterbi_batch.argtypes = [vp, vp, i64, vp, i32, i32, vp, vp, vp, vp, P(vp), P(vp), P(vp), P(vp)]
    lib.spkd_mindur_viterbi_batch.argtypes = [vp, vp, i64, vp, i32, dbl, i32, P(vp), P(vp), P(vp), P(vp)]
    lib.spkd_fb_posterior_batch.argtypes = [vp, vp, i64, vp, i32, dbl, dbl, vp, vp, vp, vp, vp, vp, vp]
    lib.spkd_gauss_models.argtypes = [vp, vp, i64, vp, vp]
    lib.spkd_gauss_loglik.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, i32, vp]
    lib.spkd_post_stats.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, i32, i64, vp]
    lib.spkd_gmm_train.argtypes = [vp, vp, i64, i64, vp, vp, vp, i32, i32, i32, dbl, vp, vp, vp]
    lib.spkd_gmm_loglik_seq.argtypes = [vp, vp, i64, vp, i32, i64, vp, i64, vp, vp, vp, vp, i32, vp]
    lib.spkd_ubm_stats.argtypes = [vp, vp, i64, vp, i32, i64, vp, vp, vp, vp, vp]
    lib.spkd_clr_link.argtypes = [vp, vp, i64, vp, vp, i32, dbl, dbl, i32, vp, vp, vp, vp, vp, vp]
    lib.spkd_feature_warp.argtypes = [vp, vp, i64, i64, vp, vp, vp, i32, vp, i64, vp, vp]
    lib.spkd_clr_identify.argtypes = [vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, i32, dbl, dbl, i32, vp, vp, vp, vp]
    lib.spkd_bw_accumulate.argtypes = [vp, vp, i64, i32, i64, vp, vp, vp, vp, vp, i64]
    lib.spkd_gw_lines.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, dbl, C.c_int, i64, vp, vp, vp, vp, vp]
    if lib.spkd_abi_version() != 2:
        raise ImportError('libspkd_hip.so ABI version mismatch')
    if path is None:
        _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _view(addr, n, dtype):
    """numpy view of n items of library-owned host memory (no copy)."""
    if not addr or n <= 0:
        return np.zeros(0, dtype=dtype)
    ct = {np.int32: C.c_int32, np.int64: C.c_int64, np.float64: C.c_double}[dtype]
    return np.ctypeslib.as_array(C.cast(C.c_void_p(addr), C.POINTER(ct)), shape=(int(n),))


def py2_roundtrip(values):
    """float(str(v)) with Python-2 str() for an array of values (host helper)."""
    v = np.ascontiguousarray(values, dtype=np.float64).copy()
    if v.size:
        load_library().spkd_py2_roundtrip(_ptr(v), v.size)
    return v


def warp_table(n):
    """The quantile table of a feature-warping window of n frames (include/spkd.h, section 10b): float32
    [2 n - 1], entry k - 1 = Phi^-1(k / (2 n)) for k = 1 .. 2 n - 1, from statistics.NormalDist in fp64 and
    rounded once.  The middle entry is exactly 0 and the table is antisymmetric about it."""
    import statistics
    n = int(n)
    if n < 1:
        raise SpkdError(SPKD_EINVAL, 'warp_table: a window of at least one frame')
    inv = statistics.NormalDist().inv_cdf
    lower = np.array([inv(k / (2.0 * n)) for k in range(1, n)], dtype=np.float64)       # (below 1/2, where k / (2 n) is exact enough)
    return np.concatenate([lower, [0.0], -lower[::-1]]).astype(np.float32)


def labels_from_merges(n, a, b):
    a = np.ascontiguousarray(a, dtype=np.int32)
    b = np.ascontiguousarray(b, dtype=np.int32)
    out = np.zeros(n, dtype=np.int32)
    st = load_library().spkd_labels_from_merges(n, len(a), _ptr(a), _ptr(b), _ptr(out))
    if st != SPKD_OK:
        raise SpkdError(st, 'bad merge log')
    return out


def count_flags(flags, off, n):
    """out[t] = number of non-zero flags among flags[off[t] : off[t] + n[t]] (host side)."""
    flags = np.ascontiguousarray(flags, dtype=np.int32)
    off = np.ascontiguousarray(off, dtype=np.int64)
    n = np.ascontiguousarray(n, dtype=np.int32)
    if len(off) != len(n):
        raise SpkdError(SPKD_EINVAL, 'one offset per group')
    if len(n) and (int((off + n).max()) > len(flags) or int(n.min()) < 0 or int(off.min()) < 0):
        raise SpkdError(SPKD_EINVAL, 'flag ranges outside the array')
    out = np.zeros(len(n), dtype=np.int32)
    st = load_library().spkd_count_flags(_ptr(flags), _ptr(off), _ptr(n), len(n), _ptr(out))
    if st != SPKD_OK:
        raise SpkdError(st, 'bad flag ranges')
    return out


def gw_lines(off, n_det, det_start, det_maxi, final_start, turn_start_s, turn_end_s, turn_begin, turn_end,
             rate, text_contract=True, want_frames=False):
    """The recipe lines of a gw() result in recipe order (spkd_gw_lines): dict with 'times'
    [n_lines, 2], 'turn' [n_lines] and, with want_frames, 'frame_b', 'frame_e', 'index'."""
    c = np.ascontiguousarray
    off = c(off, dtype=np.int64); n_det = c(n_det, dtype=np.int32)
    nt = len(n_det)
    arrs = [c(det_start, dtype=np.float64), c(det_maxi, dtype=np.float64), c(final_start, dtype=np.float64),
            c(turn_start_s, dtype=np.float64), c(turn_end_s, dtype=np.float64), c(turn_begin, dtype=np.int64),
            c(turn_end, dtype=np.int64)]
    if len(off) != nt or any(len(a) != nt for a in arrs[2:]):
        raise SpkdError(SPKD_EINVAL, 'one entry per turn')
    if nt and (int(n_det.min()) < 0 or int(off.min()) < 0 or int((off + n_det).max()) > min(len(arrs[0]), len(arrs[1]))):
        raise SpkdError(SPKD_EINVAL, 'detections outside the event arrays')
    n_lines = int(n_det.sum(dtype=np.int64)) + nt
    times = np.empty((n_lines, 2), dtype=np.float64)
    turn = np.empty(n_lines, dtype=np.int32)
    fb = np.empty(n_lines, dtype=np.int64) if want_frames else None
    fe = np.empty(n_lines, dtype=np.int64) if want_frames else None
    ix = np.empty(n_lines, dtype=np.int64) if want_frames else None
    p = lambda a: _ptr(a) if a is not None else None
    st = load_library().spkd_gw_lines(nt, _ptr(off), _ptr(n_det), *[_ptr(a) for a in arrs], float(rate),
                                      1 if text_contract else 0, n_lines, _ptr(times), p(fb), p(fe), p(ix), _ptr(turn))
    if st != SPKD_OK:
        raise SpkdError(st, 'bad growing-window result')
    return {'times': times, 'turn': turn, 'frame_b': fb, 'frame_e': fe, 'index': ix}


def vad_viterbi(scores, word_state, stay, exit_, enter):
    """Exact Viterbi over a loop of one-state words (spkd_vad_viterbi): scores [T, S] float32
    (the .lna layout), word j emitting state word_state[j], per-word fp64 constants.  Returns
    (token first frames int64, token words int32, final score)."""
    c = np.ascontiguousarray
    scores = c(scores, dtype=np.float32)
    if scores.ndim != 2:
        raise SpkdError(SPKD_EINVAL, 'scores must be [frames, states]')
    ws = c(word_state, dtype=np.int32)
    consts = [c(a, dtype=np.float64) for a in (stay, exit_, enter)]
    if any(len(a) != len(ws) for a in consts):
        raise SpkdError(SPKD_EINVAL, 'one constant of each kind per word')
    T, S = scores.shape
    tf = np.zeros(max(T, 1), dtype=np.int64)
    tw = np.zeros(max(T, 1), dtype=np.int32)
    n = C.c_int64(0)
    sc = C.c_double(0.0)
    st = load_library().spkd_vad_viterbi(T, S, _ptr(scores), len(ws), _ptr(ws), *[_ptr(a) for a in consts],
                                         _ptr(tf), _ptr(tw), C.byref(n), C.byref(sc))
    if st != SPKD_OK:
        raise SpkdError(st, 'bad decoder input')
    return tf[:n.value].copy(), tw[:n.value].copy(), sc.value


def labels_from_merges_batch(seg_off, n_merges, a, b):
    """Final 1-based cluster index of every record of every problem of an spkd_ahc
    result (same layout as its outputs)."""
    seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
    n_merges = np.ascontiguousarray(n_merges, dtype=np.int32)
    a = np.ascontiguousarray(a, dtype=np.int32)
    b = np.ascontiguousarray(b, dtype=np.int32)
    out = np.zeros(int(seg_off[-1]), dtype=np.int32)
    st = load_library().spkd_labels_from_merges_batch(len(seg_off) - 1, _ptr(seg_off), _ptr(n_merges),
                                                      _ptr(a), _ptr(b), _ptr(out))
    if st != SPKD_OK:
        raise SpkdError(st, 'bad merge log')
    return out


def _gw_capacity_ladder(turn_len, params, tight, first_guess_scale):
    """The event capacities a growing-window call is tried with (see Context.gw), as the `off`
    array of each try: with tight a quarter of the first guess, then the first guess, then the
    first guess doubled, up to 1024 times.  The caller takes the next one while the call
    answers SPKD_EOVERFLOW."""
    if not (params.rate >= 10.0 and params.winstep >= 1.0):
        raise SpkdError(SPKD_EINVAL, 'unsupported growing-window parameters (frame rate >= 10 and '
                                     'a window step of at least one frame needed)')
    # == spkd_gw_event_capacity_p(len, params), vectorised
    step = min(0.2 * params.rate, 0.5 * params.rate, params.winstep)
    full = (turn_len.astype(np.float64) / step).astype(np.int64) + 8
    if first_guess_scale != 1.0:
        full = np.maximum((full * float(first_guess_scale)).astype(np.int64), 2)
    grow = 1
    while True:
        caps = (full // 4 + 8) if tight else full * grow
        off = np.zeros(len(full) + 1, dtype=np.int64)
        off[1:] = np.cumsum(caps)
        yield off
        if tight:
            tight = False                      # an unusually busy turn: the full first guess
        elif grow < 1024:
            grow *= 2                          # a turn that re-scans (Context.gw): double until it fits
        else:
            return


class Context(object):
    """One (device, stream) context; owns nothing but the library's scratch."""

    def __init__(self, device=0, stream=None):
        """stream=None: the context owns a (blocking) stream.  stream=<handle>, 0 included:
        launch on exactly that hipStream_t (0 = the legacy default stream, which is what
        ``torch.cuda.current_stream().cuda_stream`` returns for torch's default stream)."""
        self.lib = load_library()
        h = C.c_void_p()
        if stream is None:
            st = self.lib.spkd_create(int(device), None, C.byref(h))
        else:
            st = self.lib.spkd_create_on_stream(int(device), C.c_void_p(int(stream)), C.byref(h))
        if st != SPKD_OK:
            raise SpkdError(st, 'spkd_create failed (no usable HIP device %d?)' % device)
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, 'h', None):
            for ptr, _ in self.__dict__.pop('_dev_scratch', {}).values():
                self.lib.spkd_free(self.h, C.c_void_p(ptr))
            self.lib.spkd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, st, allow=()):
        if st != SPKD_OK and st not in allow:
            raise SpkdError(st, self.lib.spkd_last_error(self.h).decode())
        return st

    def last_ms(self, which='call'):
        ms = C.c_float()
        self.check(self.lib.spkd_last_kernel_ms(self.h, TIMERS[which], C.byref(ms)))
        return ms.value

    def last_gw_items(self):
        """39x39 determinants evaluated by the most recent growing-window call."""
        n = C.c_int64()
        self.check(self.lib.spkd_last_gw_items(self.h, C.byref(n)))
        return int(n.value)

    def last_ahc_head(self):
        """Problems whose merge loops the most recent clustering call started under the others' matrices."""
        k = C.c_int64()
        self.check(self.lib.spkd_last_ahc_head(self.h, C.byref(k)))
        return int(k.value)

    # ---- device memory for torch-less hosts
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self.check(self.lib.spkd_malloc(self.h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, ptr):
        if ptr:
            self.check(self.lib.spkd_free(self.h, C.c_void_p(ptr)))

    def dev_scratch(self, name, nbytes):
        """Device buffer kept by the context and reused by later calls under the same
        name (hipMalloc / hipFree of a batch-sized buffer cost milliseconds each)."""
        cache = self.__dict__.setdefault('_dev_scratch', {})
        ptr, cap = cache.get(name, (None, 0))
        if ptr is None or cap < nbytes:
            if ptr is not None:
                self.dev_free(ptr)
            ptr, cap = self.dev_alloc(nbytes), nbytes
            cache[name] = (ptr, cap)
        return ptr

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.check(self.lib.spkd_memcpy_h2d(self.h, C.c_void_p(dptr), _ptr(arr), arr.nbytes))

    def copy_d2d(self, d_dst, d_src, nbytes):
        self.check(self.lib.spkd_memcpy_d2d(self.h, C.c_void_p(d_dst), C.c_void_p(d_src), int(nbytes)))

    def d2h(self, arr, dptr):
        assert arr.flags['C_CONTIGUOUS']
        self.check(self.lib.spkd_memcpy_d2h(self.h, _ptr(arr), C.c_void_p(dptr), arr.nbytes))

    # ---- (1)
    def set_stats(self, d_frames, n_frames, begins, ends, sets, n_sets, d_stats):
        b = np.ascontiguousarray(begins, dtype=np.int64)
        e = np.ascontiguousarray(ends, dtype=np.int64)
        s = np.ascontiguousarray(sets, dtype=np.int32)
        self.check(self.lib.spkd_set_stats(self.h, C.c_void_p(d_frames), n_frames, _ptr(b), _ptr(e),
                                           _ptr(s), len(b), n_sets, C.c_void_p(d_stats)))

    # ---- (2)
    def pair_terms(self, d_stats, ia, ib, flags=0):
        ia = np.ascontiguousarray(ia, dtype=np.int32)
        ib = np.ascontiguousarray(ib, dtype=np.int32)
        out = np.empty((len(ia), 8), dtype=np.float64)
        st = self.lib.spkd_pair_terms(self.h, C.c_void_p(d_stats), _ptr(ia), _ptr(ib), len(ia),
                                      flags, _ptr(out))
        self.check(st, allow=(SPKD_ENONFINITE,))
        return out, st

    def distance_matrix(self, kind, lambdac, d_stats, n, d_matrix):
        st = self.lib.spkd_distance_matrix(self.h, KINDS[kind], lambdac, C.c_void_p(d_stats), n,
                                           C.c_void_p(d_matrix))
        return self.check(st, allow=(SPKD_ENONFINITE,))

    # ---- (3)
    def _buf(self, name, n, dtype):
        """Host output buffer reused across calls (fresh pages cost more than the copy)."""
        cache = self.__dict__.setdefault('_bufs', {})
        arr = cache.get(name)
        if arr is None or arr.shape[0] < n or arr.dtype != np.dtype(dtype):
            arr = cache[name] = np.empty(max(n, 1), dtype=dtype)
        return arr[:n]

    def gather_stats(self, d_src, n_src, src_index, d_dst, n_dst, dst_index=None):
        """d_dst[dst_index[i]] = d_src[src_index[i]] (whole statistics records)."""
        si = np.ascontiguousarray(src_index, dtype=np.int64)
        di = None if dst_index is None else np.ascontiguousarray(dst_index, dtype=np.int64)
        self.check(self.lib.spkd_gather_stats(self.h, C.c_void_p(d_src), n_src, _ptr(si),
                                              None if di is None else _ptr(di), len(si), n_dst,
                                              C.c_void_p(d_dst)))

    def sum_stats(self, d_src, n_src, member, set_off, d_dst):
        """d_dst[s] = the sum of the records d_src[member[set_off[s] : set_off[s + 1]]], added in
        that order (spkd_sum_stats): the record of a union of frame sets from the sets' records.
        The kernel's time is last_ms('reduce_sets')."""
        m = np.ascontiguousarray(member, dtype=np.int64)
        off = np.ascontiguousarray(set_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1 or m.ndim != 1:
            raise SpkdError(SPKD_EINVAL, 'set_off: one entry per set and the total')
        if len(m) != int(off[-1]):
            raise SpkdError(SPKD_EINVAL, 'one member per entry of the sets')
        self.check(self.lib.spkd_sum_stats(self.h, C.c_void_p(d_src), int(n_src), _ptr(m), _ptr(off), len(off) - 1,
                                           C.c_void_p(d_dst)))

    def gw(self, d_frames, n_frames, begins, ends, params, log_cap=4096, tight=False, reuse=False,
           seg_stats=None, first_guess_scale=1.0):
        """Event capacity: spkd_gw_event_capacity_p is a FIRST GUESS, not a bound -- it counts
        the scans of a window end that only moves forward, but after every detection the
        reference resets the end to start + 2 * winsize (spk-change-detection.py:264-266) and
        the window regrows over frames it has already scanned: a change point found early in a
        long-grown window can make a turn need more scans than turn_len / step + 8.  The
        kernel reports that safely (SPKD_EOVERFLOW, nothing written out of bounds) and the
        call is repeated here with doubled capacities until it fits (the reference simply
        produces output for such a turn; so does this).  tight=True starts from a quarter of
        the first guess: four times less data to allocate and copy in the typical case.
        first_guess_scale (tests): scales the first guess, to exercise the doubling.
        reuse=True returns views of per-context buffers: valid until the next gw call
        on this context.
        seg_stats: a callable n_records -> device pointer; turns the call into the fused
        form (spkd_gw_fused): the statistics record of segment j of turn t is left at
        record off[t] + j of that buffer."""
        b = np.ascontiguousarray(begins, dtype=np.int64)
        e = np.ascontiguousarray(ends, dtype=np.int64)
        nt = len(b)
        for off in _gw_capacity_ladder(e - b, params, tight, first_guess_scale):
            nev = int(off[-1])
            mk = self._buf if reuse else (lambda name, n, dt: np.empty(n, dtype=dt))
            n_win = mk('n_win', nt, np.int32)
            win_maxd = mk('win_maxd', nev, np.float64)
            win_det = mk('win_det', nev, np.int32)
            det_start = mk('det_start', nev, np.float64)
            det_maxi = mk('det_maxi', nev, np.float64)
            det_d = mk('det_d', nev, np.float64)
            final_start = mk('final_start', nt, np.float64)
            d_seg = None if seg_stats is None else seg_stats(nev)
            while True:
                log = (CandLog * max(log_cap, 1))()
                cnt = C.c_int64(0)
                if seg_stats is None:
                    st = self.lib.spkd_gw_ex(self.h, C.c_void_p(d_frames), n_frames, _ptr(b), _ptr(e), nt,
                                             C.byref(params), _ptr(off), 0, _ptr(n_win),
                                             _ptr(win_maxd), _ptr(win_det), _ptr(det_start), _ptr(det_maxi),
                                             _ptr(det_d), _ptr(final_start), C.cast(log, C.c_void_p), log_cap,
                                             C.byref(cnt))
                else:
                    st = self.lib.spkd_gw_fused(self.h, C.c_void_p(d_frames), n_frames, _ptr(b), _ptr(e), nt,
                                                C.byref(params), _ptr(off), 0, _ptr(n_win),
                                                _ptr(win_maxd), _ptr(win_det), _ptr(det_start), _ptr(det_maxi),
                                                _ptr(det_d), _ptr(final_start), C.c_void_p(d_seg),
                                                C.cast(log, C.c_void_p), log_cap, C.byref(cnt))
                if not (st == SPKD_EOVERFLOW and cnt.value > log_cap):
                    break
                log_cap = int(cnt.value) + 16      # the run is deterministic: retry with room
            if st != SPKD_EOVERFLOW:
                break
        self.check(st, allow=(SPKD_ENONFINITE,))
        return dict(status=st, off=off, n_ev=nev, n_win=n_win, win_maxd=win_maxd, win_det=win_det,
                    det_start=det_start, det_maxi=det_maxi, det_d=det_d, final_start=final_start,
                    log=log, log_count=min(int(cnt.value), log_cap))

    def gw_batch(self, d_frames, n_frames, begins, ends, params, turn_start_s, turn_end_s, file_off, file_len,
                 seg_stats, tight=True, first_guess_scale=1.0, want_index=False):
        """The batch hand-off (spkd_gw_batch): gw(seg_stats=...) whose results come back as recipe
        lines -- times after the 12-digit round trip, turn, the frame range each fused record
        covers -- plus the redo list, the lines whose range the round trip moved.  The arrays are
        views of memory the context owns: valid until the next gw_batch on it.  Capacities as
        in gw(): a first guess that doubles until it fits."""
        c = np.ascontiguousarray
        b = c(begins, dtype=np.int64)
        e = c(ends, dtype=np.int64)
        nt = len(b)
        host = [c(turn_start_s, dtype=np.float64), c(turn_end_s, dtype=np.float64), c(file_off, dtype=np.int64),
                c(file_len, dtype=np.int64)]
        if any(len(a) != nt for a in host):
            raise SpkdError(SPKD_EINVAL, 'one entry per turn')
        view = GwLinesView()
        for off in _gw_capacity_ladder(e - b, params, tight, first_guess_scale):
            nev = int(off[-1])
            d_seg = seg_stats(nev)
            st = self.lib.spkd_gw_batch(self.h, C.c_void_p(d_frames), n_frames, _ptr(b), _ptr(e), nt, C.byref(params),
                                        _ptr(off), *[_ptr(a) for a in host], C.c_void_p(d_seg),
                                        1 if want_index else 0, C.byref(view))
            if st != SPKD_EOVERFLOW:
                break
        self.check(st, allow=(SPKD_ENONFINITE,))
        n, nr = int(view.n_lines), int(view.n_redo)
        return dict(status=st, off=off, n_ev=nev, d_seg=d_seg, n_lines=n, n_win=_view(view.n_win, nt if n else 0, np.int32),
                    times=_view(view.times, 2 * n, np.float64).reshape(-1, 2), turn=_view(view.turn, n, np.int32),
                    frame_b=_view(view.frame_b, n, np.int64), frame_e=_view(view.frame_e, n, np.int64),
                    index=_view(view.index, n, np.int64) if want_index else None, d_index=view.d_index,
                    redo_line=_view(view.redo_line, nr, np.int64), redo_begin=_view(view.redo_begin, nr, np.int64),
                    redo_end=_view(view.redo_end, nr, np.int64))

    def ahc_fused(self, d_frames, n_frames, d_records, n_records, d_line_index, seg_off, redo_line, redo_begin,
                  redo_end, params):
        """spkd_ahc_fused: redo statistics, working copies read through the line -> record map,
        matrix, merge loop and label replay in one call.  The arrays are views of memory the
        context owns: valid until the next ahc_fused on it."""
        c = np.ascontiguousarray
        seg_off = c(seg_off, dtype=np.int64)
        rl, rb, re_ = c(redo_line, dtype=np.int64), c(redo_begin, dtype=np.int64), c(redo_end, dtype=np.int64)
        if not (len(rl) == len(rb) == len(re_)):
            raise SpkdError(SPKD_EINVAL, 'one range per redo line')
        npb, nt = len(seg_off) - 1, int(seg_off[-1])
        out = [C.c_void_p() for _ in range(5)]
        st = self.lib.spkd_ahc_fused(self.h, C.c_void_p(d_frames), n_frames, C.c_void_p(d_records), n_records,
                                     C.c_void_p(d_line_index), _ptr(seg_off), npb, _ptr(rl), _ptr(rb), _ptr(re_), len(rl),
                                     C.byref(params), *[C.byref(o) for o in out])
        self.check(st, allow=(SPKD_ENONFINITE,))
        if st != SPKD_OK:
            return dict(status=st)
        return dict(status=st, n_merges=_view(out[0].value, npb, np.int32), a=_view(out[1].value, nt, np.int32),
                    b=_view(out[2].value, nt, np.int32), d=_view(out[3].value, nt, np.float64),
                    labels=_view(out[4].value, nt, np.int32))

    def sw(self, d_frames, n_frames, begins, ends, params):
        b = np.ascontiguousarray(begins, dtype=np.int64)
        e = np.ascontiguousarray(ends, dtype=np.int64)
        nt = len(b)
        cnt = [self.lib.spkd_sw_window_count(int(e[t] - b[t]), params.winsize, params.winstep)
               for t in range(nt)]
        if any(c < 0 for c in cnt):
            raise SpkdError(SPKD_EINVAL, 'window size and step must be at least one frame')
        off = np.zeros(nt + 1, dtype=np.int64)
        off[1:] = np.cumsum(cnt)
        d = np.zeros(int(off[-1]), dtype=np.float64)
        st = self.lib.spkd_sw(self.h, C.c_void_p(d_frames), n_frames, _ptr(b), _ptr(e), nt,
                              C.byref(params), _ptr(off), _ptr(d))
        self.check(st, allow=(SPKD_ENONFINITE,))
        return st, off, d

    @staticmethod
    def _sw_outputs(d_off, ev_off):
        """ev_off (None: the bound, windows // 2 + 1 slots per turn) and the output arrays of the
        positive-run pass, in the order the two calls take them."""
        nt = len(d_off) - 1
        if ev_off is None:
            ev_off = np.zeros(nt + 1, dtype=np.int64)
            ev_off[1:] = np.cumsum(np.diff(d_off) // 2 + 1)
        ev_off = np.ascontiguousarray(ev_off, dtype=np.int64)
        if len(ev_off) != nt + 1:
            raise SpkdError(SPKD_EINVAL, 'one event offset per turn and the total')
        nev = max(int(ev_off[-1]), 0)
        out = dict(n_det=np.zeros(nt, dtype=np.int32), det_start=np.zeros(nev), det_maxi=np.zeros(nev),
                   det_d=np.zeros(nev), final_start=np.zeros(nt), win_cnt=np.zeros(nt, dtype=np.int64),
                   win_max=np.zeros(nt), win_min=np.zeros(nt), det_max=np.zeros(nt), det_min=np.zeros(nt))
        return ev_off, out

    def sw_runs(self, d_dist, d_off, params, ev_off=None):
        """The positive-run pass of dist_sw (spkd_sw_runs) over the device array d_dist, turn t
        owning [d_off[t], d_off[t+1]) -> dict: off (event offsets), n_det, final_start and the
        summary counters per turn, det_start / det_maxi / det_d per event slot, status."""
        d_off = np.ascontiguousarray(d_off, dtype=np.int64)
        if d_off.ndim != 1 or len(d_off) < 1:
            raise SpkdError(SPKD_EINVAL, 'd_off: one entry per turn and the total')
        ev_off, out = self._sw_outputs(d_off, ev_off)
        st = self.lib.spkd_sw_runs(self.h, C.c_void_p(d_dist), _ptr(d_off), len(d_off) - 1, C.byref(params),
                                   _ptr(ev_off), *[_ptr(a) for a in out.values()])
        self.check(st)
        return dict(out, status=st, off=ev_off, d_off=d_off)

    def sw_batch(self, d_frames, n_frames, begins, ends, params, tile_windows=0, want_d=False, d_off=None,
                 ev_off=None):
        """Sliding-window change detection of every turn in one call (spkd_sw_batch): the result
        of sw_runs over the distances of sw(), which stay on the device unless want_d ('d').
        d_off / ev_off: None for the window counts / the bound (tests pass their own)."""
        b = np.ascontiguousarray(begins, dtype=np.int64)
        e = np.ascontiguousarray(ends, dtype=np.int64)
        nt = len(b)
        if d_off is None:
            cnt = [self.lib.spkd_sw_window_count(int(n), params.winsize, params.winstep) for n in (e - b).tolist()]
            if any(c < 0 for c in cnt):
                raise SpkdError(SPKD_EINVAL, 'window size and step must be at least one frame')
            d_off = np.zeros(nt + 1, dtype=np.int64)
            d_off[1:] = np.cumsum(cnt)
        d_off = np.ascontiguousarray(d_off, dtype=np.int64)
        if len(d_off) != nt + 1:
            raise SpkdError(SPKD_EINVAL, 'one window offset per turn and the total')
        ev_off, out = self._sw_outputs(d_off, ev_off)
        d = np.zeros(max(int(d_off[-1]), 0), dtype=np.float64) if want_d else None
        st = self.lib.spkd_sw_batch(self.h, C.c_void_p(d_frames), n_frames, _ptr(b), _ptr(e), nt, C.byref(params),
                                    _ptr(d_off), _ptr(ev_off), int(tile_windows), *[_ptr(a) for a in out.values()],
                                    None if d is None else _ptr(d))
        self.check(st, allow=(SPKD_ENONFINITE,))
        return dict(out, status=st, off=ev_off, d_off=d_off, d=d)

    def merge_batch(self, d_frames, n_frames, line_off, begins, ends, kind, lambdac, threshold, flags=0):
        """merge_rec (`-m m`) for every problem of line_off in one call (spkd_merge_batch), each as
        a run of the script on its lines alone -> dict: merged (1: the line joined the run before
        it, 0: it starts one, -1 behind a stop) and dist per line, n_done and the script's counters
        (win_cnt, win_max, win_min, det_cnt, det_max, det_min) per problem, status.  status is
        SPKD_ENONFINITE when a covariance with infs or NaNs stopped a problem (n_done[p] < its
        size); the other problems are complete.  flags: MERGE_NO_AHEAD."""
        line_off = np.ascontiguousarray(line_off, dtype=np.int64)
        if line_off.ndim != 1 or len(line_off) < 1:
            raise SpkdError(SPKD_EINVAL, 'line_off: one entry per problem and the total')
        b = np.ascontiguousarray(begins, dtype=np.int64)
        e = np.ascontiguousarray(ends, dtype=np.int64)
        npb = len(line_off) - 1
        nt = max(int(line_off[-1]), 0)
        if len(b) != nt or len(e) != nt:
            raise SpkdError(SPKD_EINVAL, 'one frame range per line')
        out = dict(merged=np.zeros(nt, dtype=np.int32), dist=np.full(nt, np.nan), n_done=np.zeros(npb, dtype=np.int64),
                   win_cnt=np.zeros(npb, dtype=np.int64), win_max=np.zeros(npb), win_min=np.zeros(npb),
                   det_cnt=np.zeros(npb, dtype=np.int64), det_max=np.zeros(npb), det_min=np.zeros(npb))
        st = self.lib.spkd_merge_batch(self.h, C.c_void_p(d_frames), int(n_frames), npb, _ptr(line_off), _ptr(b), _ptr(e),
                                       KINDS[kind] if isinstance(kind, str) else int(kind), float(lambdac),
                                       float(threshold), int(flags), *[_ptr(a) for a in out.values()])
        self.check(st, allow=(SPKD_ENONFINITE,))
        return dict(out, status=st)

    # ---- (6)
    def mfcc(self, d_pcm, n_samples, params, melfb, dct, mean, scale, transform, d_features):
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (melfb, dct, mean, scale, transform)]
        n = C.c_int64(0)
        self.check(self.lib.spkd_mfcc(self.h, C.c_void_p(d_pcm), n_samples, C.byref(params), *[_ptr(a) for a in arrs],
                                      C.c_void_p(d_features), C.byref(n)))
        return int(n.value)

    def mfcc_batch(self, d_pcm, sample_off, params, melfb, dct, mean, scale, transform, d_features):
        """The front-end for every file of concatenated device samples (spkd_mfcc_batch): file f owns
        the samples [sample_off[f], sample_off[f+1]); its features land at the rows [frame_off[f],
        frame_off[f+1]) of d_features.  Returns frame_off (int64, one entry per file and the total)."""
        off = np.ascontiguousarray(sample_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise SpkdError(SPKD_EINVAL, 'sample_off: one entry per file and the total')
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (melfb, dct, mean, scale, transform)]
        frame_off = np.zeros(len(off), dtype=np.int64)
        self.check(self.lib.spkd_mfcc_batch(self.h, C.c_void_p(d_pcm), len(off) - 1, _ptr(off), C.byref(params),
                                            *[_ptr(a) for a in arrs], C.c_void_p(d_features), _ptr(frame_off)))
        return frame_off

    # ---- (6b)
    def resample_batch(self, d_in, in_off, channels, conv, convs, taps, d_out):
        """Interleaved int16 files on the device -> mono int16 at one rate (spkd_resample_batch):
        file f owns the elements [in_off[f], in_off[f+1]) of d_in, has channels[f] channels and the
        conversion convs[conv[f]] (ResampleConv, or (up, down, half_taps, taps_off)); taps: every
        conversion's float32 table, concatenated.  Its samples land at [out_off[f], out_off[f+1])
        of d_out.  Returns out_off (int64, one entry per file and the total)."""
        off = np.ascontiguousarray(in_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise SpkdError(SPKD_EINVAL, 'in_off: one entry per file and the total')
        ch = np.ascontiguousarray(channels, dtype=np.int32)
        cv = np.ascontiguousarray(conv, dtype=np.int32)
        if ch.shape != (len(off) - 1,) or cv.shape != ch.shape:
            raise SpkdError(SPKD_EINVAL, 'channels, conv: one entry per file')
        table = (ResampleConv * max(len(convs), 1))(*[v if isinstance(v, ResampleConv) else ResampleConv(*[int(x) for x in v])
                                                      for v in convs])
        taps = np.ascontiguousarray(taps, dtype=np.float32).ravel()
        out_off = np.zeros(len(off), dtype=np.int64)
        self.check(self.lib.spkd_resample_batch(self.h, C.c_void_p(d_in), len(off) - 1, _ptr(off), _ptr(ch), _ptr(cv),
                                                len(convs), table, _ptr(taps) if taps.size else None,
                                                C.c_void_p(d_out), _ptr(out_off)))
        return out_off

    # ---- (6b2) delay-and-sum beamforming
    @staticmethod
    def _bf_files(in_off, channels, geom, geoms):
        off = np.ascontiguousarray(in_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise SpkdError(SPKD_EINVAL, 'in_off: one entry per file and the total')
        ch = np.ascontiguousarray(channels, dtype=np.int32)
        gi = np.ascontiguousarray(geom, dtype=np.int32)
        if ch.shape != (len(off) - 1,) or gi.shape != ch.shape:
            raise SpkdError(SPKD_EINVAL, 'channels, geom: one entry per file')
        table = (BfGeom * max(len(geoms), 1))(*[g if isinstance(g, BfGeom) else BfGeom(*[int(x) for x in g]) for g in geoms])
        return off, ch, gi, table

    def bf_gcc(self, d_in, in_off, channels, geom, geoms, ref, d_ref, d_lag, d_val, d_curve=None):
        """GCC-PHAT candidates of every step and channel (spkd_bf_gcc): file f owns the elements
        [in_off[f], in_off[f+1]) of d_in, has channels[f] channels, the geometry geoms[geom[f]] (BfGeom,
        or (hop, window, max_lag)) and the reference channel ref[f] (-1: the loudest).  d_ref gets the
        reference channel per file, d_lag / d_val the BF_NBEST candidates at 4 (wg_off[f] + t C + c),
        wg_off the running sum of T C; d_curve, if given, every correlation value.  Returns (step_off,
        curve_off), int64 with one entry per file and the total.  Time: last_ms('bf_gcc')."""
        off, ch, gi, table = self._bf_files(in_off, channels, geom, geoms)
        rf = np.ascontiguousarray(ref, dtype=np.int32)
        if rf.shape != ch.shape:
            raise SpkdError(SPKD_EINVAL, 'ref: one entry per file')
        step_off = np.zeros(len(off), dtype=np.int64)
        curve_off = np.zeros(len(off), dtype=np.int64)
        self.check(self.lib.spkd_bf_gcc(self.h, C.c_void_p(d_in), len(off) - 1, _ptr(off), _ptr(ch), _ptr(gi), len(geoms), table,
                                        _ptr(rf), C.c_void_p(d_ref), C.c_void_p(d_lag), C.c_void_p(d_val),
                                        C.c_void_p(d_curve) if d_curve else None, _ptr(step_off), _ptr(curve_off)))
        return step_off, curve_off

    def bf_track(self, step_off, channels, d_lag, d_val, n_best, min_peak, jump_penalty, jump_cap, d_delay):
        """One delay per step and channel from the candidates (spkd_bf_track): d_delay int32 at
        wg_off[f] + t C + c.  Time: last_ms('bf_track')."""
        off = np.ascontiguousarray(step_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise SpkdError(SPKD_EINVAL, 'step_off: one entry per file and the total')
        ch = np.ascontiguousarray(channels, dtype=np.int32)
        if ch.shape != (len(off) - 1,):
            raise SpkdError(SPKD_EINVAL, 'channels: one entry per file')
        self.check(self.lib.spkd_bf_track(self.h, len(off) - 1, _ptr(off), _ptr(ch), C.c_void_p(d_lag), C.c_void_p(d_val),
                                          int(n_best), float(min_peak), float(jump_penalty), int(jump_cap), C.c_void_p(d_delay)))

    def bf_sum(self, d_in, in_off, channels, geom, geoms, d_delay, d_out):
        """The channels summed at their delays (spkd_bf_sum) -> mono int16 at d_out, a file's n frames at
        [out_off[f], out_off[f+1]).  Returns out_off.  Time: last_ms('bf_sum')."""
        off, ch, gi, table = self._bf_files(in_off, channels, geom, geoms)
        out_off = np.zeros(len(off), dtype=np.int64)
        self.check(self.lib.spkd_bf_sum(self.h, C.c_void_p(d_in), len(off) - 1, _ptr(off), _ptr(ch), _ptr(gi), len(geoms), table,
                                        C.c_void_p(d_delay), C.c_void_p(d_out), _ptr(out_off)))
        return out_off

    # ---- (6b3) the delay stream
    def tdoa_pack(self, d_delay, d_val, min_peak, n, d_out):
        """n entries of the delay stream from what spkd_bf_track read and wrote (spkd_tdoa_pack): d_out[i] =
        d_delay[i] where the first candidate's value d_val[4 i] >= min_peak, TDOA_NONE elsewhere.  Time:
        last_ms('tdoa_pack')."""
        self.check(self.lib.spkd_tdoa_pack(self.h, C.c_void_p(d_delay), C.c_void_p(d_val), float(min_peak), int(n),
                                           C.c_void_p(d_out)))

    @staticmethod
    def _tdoa_stream(stream):
        """(d_stream, n_entries, file table [n_files, TDOA_FILE] int64, (hop, window, rate_out)) -> the arguments of
        spkd_tdoa_stats from d_stream to rate_out; a pointer keeps its array."""
        d_stream, n_entries, table, clock = stream
        table = np.ascontiguousarray(table, dtype=np.int64)
        if table.ndim != 2 or table.shape[1] != TDOA_FILE:
            raise SpkdError(SPKD_EINVAL, 'the delay stream\'s file table: [n_files, %d] int64' % TDOA_FILE)
        hop, window, rate_out = (int(v) for v in clock)
        return (C.c_void_p(d_stream), int(n_entries), _ptr(table), len(table), hop, window, rate_out), table

    def tdoa_stats(self, stream, begins, ends, files, sets, n_sets, d_stats):
        """The exact delay statistics of frame sets (spkd_tdoa_stats): stream as _tdoa_stream takes it; the frame
        ranges [begins, ends) of the batch, each with its file and its set, the sets ascending; d_stats int64
        [n_sets, 8, 3], per channel (n, sum x, sum x^2).  Time: last_ms('tdoa_stats')."""
        args, _keep = self._tdoa_stream(stream)
        b, e = np.ascontiguousarray(begins, dtype=np.int64), np.ascontiguousarray(ends, dtype=np.int64)
        f, s = np.ascontiguousarray(files, dtype=np.int32), np.ascontiguousarray(sets, dtype=np.int32)
        if any(a.ndim != 1 for a in (b, e, f, s)) or not (len(b) == len(e) == len(f) == len(s)):
            raise SpkdError(SPKD_EINVAL, 'one begin, end, file and set per range')
        self.check(self.lib.spkd_tdoa_stats(self.h, *args, _ptr(b), _ptr(e), _ptr(f), _ptr(s), len(b), int(n_sets),
                                            C.c_void_p(d_stats)))

    def tdoa_cuts(self, stream, begins, ends, files, min_piece, min_frames, floor_s, lambdac, threshold):
        """The best seat cut of every frame range (spkd_tdoa_cuts; include/spkd.h (6b4)): stream as _tdoa_stream takes
        it, the ranges [begin, end) in the batch's numbering, each with its file.  Returns (cut int64 [n]: the frame,
        -1 for none; delta float64 [n]: the highest Delta of the range, NaN when none is defined).  Time:
        last_ms('tdoa_cuts')."""
        args, _keep = self._tdoa_stream(stream)
        b = np.ascontiguousarray(begins, dtype=np.int64)
        e = np.ascontiguousarray(ends, dtype=np.int64)
        f = np.ascontiguousarray(files, dtype=np.int32)
        if not (b.ndim == 1 and len(b) == len(e) == len(f)):
            raise SpkdError(SPKD_EINVAL, 'one begin, end and file per range')
        cut, delta = np.full(len(b), -1, dtype=np.int64), np.full(len(b), np.nan)
        self.check(self.lib.spkd_tdoa_cuts(self.h, *args, _ptr(b), _ptr(e), _ptr(f), len(b), int(min_piece), int(min_frames),
                                           float(floor_s), float(lambdac), float(threshold), _ptr(cut), _ptr(delta)))
        return cut, delta

    def tdoa_split(self, d_stats, off, prob_file, table, clock, min_frames, floor_s, lambdac, threshold):
        """One agglomerative chain per problem over the delay records at d_stats (spkd_tdoa_split): problem p owns the
        records off[p] .. off[p + 1] and is of file prob_file[p] of table, the stream's file table; clock = (hop,
        window, rate_out).  Returns dict(n_merges int32 [problems], a, b int32 [n], d float64 [n], placed int32 [n]):
        the log of problem p at off[p], in spkd_ahc's convention (labels_from_merges_batch replays it).  Time:
        last_ms('tdoa_split')."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        pf = np.ascontiguousarray(prob_file, dtype=np.int32)
        table = np.ascontiguousarray(table, dtype=np.int64)
        if table.ndim != 2 or table.shape[1] != TDOA_FILE:
            raise SpkdError(SPKD_EINVAL, 'the delay stream\'s file table: [n_files, %d] int64' % TDOA_FILE)
        if off.ndim != 1 or len(off) != len(pf) + 1:
            raise SpkdError(SPKD_EINVAL, 'one file per problem and one offset more')
        n = max(int(off[-1]), 0)
        a, b, d = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)
        nm, placed = np.zeros(len(pf), dtype=np.int32), np.zeros(n, dtype=np.int32)
        hop, window, rate_out = (int(v) for v in clock)
        self.check(self.lib.spkd_tdoa_split(self.h, C.c_void_p(d_stats), len(pf), _ptr(off), _ptr(pf), _ptr(table), len(table),
                                            hop, window, rate_out, int(min_frames), float(floor_s), float(lambdac),
                                            float(threshold), _ptr(a), _ptr(b), _ptr(d), _ptr(nm), _ptr(placed)))
        return dict(n_merges=nm, a=a, b=b, d=d, placed=placed)

    def tdoa_models(self, d_stats, spk_file, ok, table, min_frames, floor_s, d_models):
        """One Gaussian per (speaker, channel) from d_stats (spkd_tdoa_models) into d_models double [n, 8,
        TDOA_MODEL]; spk_file: the speakers' files, ascending; ok: their acoustic models; table: the stream's file
        table.  Returns live (int32 [n_files]): bit c set where channel c has min_frames reliable frames for every
        speaker of the file that is ok.  Time: last_ms('tdoa_models')."""
        table = np.ascontiguousarray(table, dtype=np.int64)
        if table.ndim != 2 or table.shape[1] != TDOA_FILE:
            raise SpkdError(SPKD_EINVAL, 'the delay stream\'s file table: [n_files, %d] int64' % TDOA_FILE)
        sf, ok = np.ascontiguousarray(spk_file, dtype=np.int32), np.ascontiguousarray(ok, dtype=np.int32)
        if sf.ndim != 1 or sf.shape != ok.shape:
            raise SpkdError(SPKD_EINVAL, 'one file and one ok flag per speaker')
        live = np.zeros(len(table), dtype=np.int32)
        self.check(self.lib.spkd_tdoa_models(self.h, C.c_void_p(d_stats), len(sf), _ptr(sf), _ptr(ok), _ptr(table), len(table),
                                             int(min_frames), float(floor_s), C.c_void_p(d_models), _ptr(live)))
        return live

    def tdoa_score(self, stream, d_models, n_models, live, seq_begin, seq_end, seq_file, seq_model, seq_n_models, n_cols,
                   weight, d_scores):
        """weight times the delay log-likelihood added to the scores gauss_loglik (or gmm_loglik_seq) left at
        d_scores (spkd_tdoa_score): the same sequences, each with its file; live as tdoa_models returned it.  Entries
        that are not finite and columns past a sequence's models keep their bits.  Time: last_ms('tdoa_score')."""
        args, _keep = self._tdoa_stream(stream)
        c = np.ascontiguousarray
        lv = c(live, dtype=np.int32)
        b, e = c(seq_begin, dtype=np.int64), c(seq_end, dtype=np.int64)
        f, m, k = c(seq_file, dtype=np.int32), c(seq_model, dtype=np.int32), c(seq_n_models, dtype=np.int32)
        if any(a.ndim != 1 for a in (lv, b, e, f, m, k)) or not (len(b) == len(e) == len(f) == len(m) == len(k)) \
                or len(lv) != len(_keep):
            raise SpkdError(SPKD_EINVAL, 'one begin, end, file, first model and model count per sequence; one live mask per file')
        self.check(self.lib.spkd_tdoa_score(self.h, *args, C.c_void_p(d_models), int(n_models), _ptr(lv), len(b), _ptr(b),
                                            _ptr(e), _ptr(f), _ptr(m), _ptr(k), int(n_cols), float(weight),
                                            C.c_void_p(d_scores)))

    # ---- (6b5) overlapped speech from the delay stream
    def tdoa_second(self, d_delay, d_lag, d_val, n_best, min_peak, min_second, guard, n, d_out):
        """n entries of the runner-up stream from what spkd_bf_track read and wrote (spkd_tdoa_second): d_out[i] = the lag
        of the first of the n_best candidates with a finite value that lies more than guard samples from d_delay[i],
        if its value >= min_second and the step is reliable (d_val[4 i] >= min_peak); TDOA_NONE elsewhere.  Time:
        last_ms('tdoa_second')."""
        self.check(self.lib.spkd_tdoa_second(self.h, C.c_void_p(d_delay), C.c_void_p(d_lag), C.c_void_p(d_val), int(n_best),
                                             float(min_peak), float(min_second), int(guard), int(n), C.c_void_p(d_out)))

    def tdoa_overlap(self, stream, d_second, d_models, live, spk_off, gate, min_channels, min_steps, d_pair):
        """The pair of speakers of every step (spkd_tdoa_overlap; include/spkd.h (6b5)): stream as _tdoa_stream takes it,
        d_second the runner-up stream of the same layout, d_models and live as tdoa_models left them, spk_off int64
        [n_files + 1] the first model of every file.  d_pair int32 [sum T, 2]: per step (j, k), j < k counted from the
        file's first model, or (-1, -1).  Time: last_ms('tdoa_overlap'), both launches."""
        args, _keep = self._tdoa_stream(stream)
        lv = np.ascontiguousarray(live, dtype=np.int32)
        so = np.ascontiguousarray(spk_off, dtype=np.int64)
        if lv.shape != (len(_keep),) or so.shape != (len(_keep) + 1,):
            raise SpkdError(SPKD_EINVAL, 'one live mask per file, and one speaker offset per file and the total')
        self.check(self.lib.spkd_tdoa_overlap(self.h, *args, C.c_void_p(d_second), C.c_void_p(d_models), _ptr(lv), _ptr(so),
                                              float(gate), int(min_channels), int(min_steps), C.c_void_p(d_pair)))

    # ---- (6c) the seed stage of the self-trained detector
    def frame_energy_batch(self, d_pcm, sample_off, hop, window, d_energy):
        """The energy of every frame of concatenated device samples (spkd_frame_energy_batch): file f
        owns the samples [sample_off[f], sample_off[f+1]) and has len // hop frames, mfcc_batch's
        clock; frame t covers the file's samples t * hop .. t * hop + window - 1 (0 past its end) and
        d_energy[frame] = window * sum s^2 - (sum s)^2 as int64, exact.  Returns frame_off (int64, one
        entry per file and the total).  The kernel's time is last_ms('frame_energy')."""
        off = np.ascontiguousarray(sample_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise SpkdError(SPKD_EINVAL, 'sample_off: one entry per file and the total')
        frame_off = np.zeros(len(off), dtype=np.int64)
        self.check(self.lib.spkd_frame_energy_batch(self.h, C.c_void_p(d_pcm), _ptr(off), len(off) - 1, int(hop), int(window),
                                                    C.c_void_p(d_energy), _ptr(frame_off)))
        return frame_off

    def energy_seeds(self, d_energy, frame_off, k_low, k_high):
        """Per file of concatenated device energies (int64 [sum T]) the k_low[f]-th smallest and the
        k_high[f]-th largest (1-based) and the runs of frames at or beyond them (spkd_energy_seeds)
        -> (lo int64 [n], hi int64 [n], seeded int32 [n], run_off int64 [2 n + 1], run_begin,
        run_end): the runs of file f and class c (0: E <= lo, 1: E >= hi) at [run_off[2 f + c],
        run_off[2 f + c + 1]), absolute frames [begin, end), ascending; a file with a k outside
        [1, T] or lo >= hi is not seeded and has none.  Copies: the library's arrays live until the
        next call.  The kernels' time is last_ms('energy_seeds')."""
        off = self._frame_off(frame_off)
        n = len(off) - 1
        kl, kh = np.ascontiguousarray(k_low, dtype=np.int64), np.ascontiguousarray(k_high, dtype=np.int64)
        if kl.shape != (n,) or kh.shape != (n,):
            raise SpkdError(SPKD_EINVAL, 'k_low, k_high: one entry per file')
        lo, hi, seeded = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32)
        out = [C.c_void_p() for _ in range(3)]
        self.check(self.lib.spkd_energy_seeds(self.h, C.c_void_p(d_energy), _ptr(off), n, _ptr(kl), _ptr(kh), _ptr(lo),
                                              _ptr(hi), _ptr(seeded), *[C.byref(o) for o in out]))
        run_off = _view(out[0].value, 2 * n + 1, np.int64).copy()
        n_runs = int(run_off[-1])
        return (lo, hi, seeded, run_off, _view(out[1].value, n_runs, np.int64).copy(),
                _view(out[2].value, n_runs, np.int64).copy())

    # ---- (7)
    def gmm_loglik(self, d_features, n_frames, gmm, d_scores):
        """Per-frame state log-likelihoods of device features [n_frames, 39] into device
        scores [n_frames, n_states]; gmm: a dict of host arrays (mean, inv_var, log_norm
        float32; state_off, kernel int32; log_weight float32)."""
        a = {k: np.ascontiguousarray(gmm[k], dtype=np.int32 if k in ('state_off', 'kernel') else np.float32)
             for k in ('mean', 'inv_var', 'log_norm', 'state_off', 'kernel', 'log_weight')}
        K, S = len(a['log_norm']), len(a['state_off']) - 1
        if a['mean'].size != K * DIM or a['inv_var'].size != K * DIM or S < 1 or \
                len(a['kernel']) != len(a['log_weight']) or int(a['state_off'][-1]) != len(a['kernel']):
            raise SpkdError(SPKD_EINVAL, 'inconsistent model array sizes')
        p = GmmParams(K, S, a['mean'].shape[-1] if a['mean'].ndim == 2 else DIM,
                      *[_ptr(a[k]) for k in ('mean', 'inv_var', 'log_norm', 'state_off', 'kernel', 'log_weight')])
        self.check(self.lib.spkd_gmm_loglik(self.h, C.c_void_p(d_features), int(n_frames), C.byref(p),
                                            C.c_void_p(d_scores)))

    # ---- (7b) the decision part for a batch of files
    @staticmethod
    def _frame_off(frame_off):
        off = np.ascontiguousarray(frame_off, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1:
            raise SpkdError(SPKD_EINVAL, 'frame_off: one entry per file and the total')
        return off

    @staticmethod
    def _tokens(out, n):
        """Copies of the four arrays that a decoder handed back for n files."""
        tok_off = _view(out[0].value, n + 1, np.int64).copy()
        n_tok = int(tok_off[-1])
        return (tok_off, _view(out[1].value, n_tok, np.int64).copy(), _view(out[2].value, n_tok, np.int32).copy(),
                _view(out[3].value, n, np.float64).copy())

    @staticmethod
    def _seq_args(model_ok, seq_begin, seq_end, seq_model, seq_n_models):
        """-> (the arguments of spkd_gauss_loglik from n_models to h_seq_n_models, frame_off); a pointer keeps its array."""
        c = np.ascontiguousarray
        ok = c(model_ok, dtype=np.int32)
        b, e = c(seq_begin, dtype=np.int64), c(seq_end, dtype=np.int64)
        m, k = c(seq_model, dtype=np.int32), c(seq_n_models, dtype=np.int32)
        if any(a.ndim != 1 for a in (ok, b, e, m, k)) or not (len(b) == len(e) == len(m) == len(k)):
            raise SpkdError(SPKD_EINVAL, 'one begin, end, first model and model count per sequence')
        frame_off = np.zeros(len(b) + 1, dtype=np.int64)
        frame_off[1:] = np.cumsum(e - b)
        return (len(ok), _ptr(ok), len(b), _ptr(b), _ptr(e), _ptr(m), _ptr(k)), frame_off

    @staticmethod
    def _range_sets(set_off, range_begin, range_end):
        """-> the arguments of spkd_gmm_train from n_speakers to h_range_end; a pointer keeps its array."""
        c = np.ascontiguousarray
        off, b, e = c(set_off, dtype=np.int64), c(range_begin, dtype=np.int64), c(range_end, dtype=np.int64)
        if off.ndim != 1 or len(off) < 1 or b.ndim != 1 or e.ndim != 1:
            raise SpkdError(SPKD_EINVAL, 'set_off: one entry per speaker and the total')
        if not (len(b) == len(e) == int(off[-1])):
            raise SpkdError(SPKD_EINVAL, 'one begin and end per range of the sets')
        return len(off) - 1, _ptr(off), _ptr(b), _ptr(e)

    def vad_shift_batch(self, d_scores, frame_off, n_states, shift, d_out=None):
        """shift_dec_bord for every file of concatenated device scores [sum T, n_states]
        (spkd_vad_shift_batch); d_out=None: in place."""
        off = self._frame_off(frame_off)
        self.check(self.lib.spkd_vad_shift_batch(self.h, C.c_void_p(d_scores), len(off) - 1, _ptr(off), int(n_states),
                                                 float(shift), C.c_void_p(d_scores if d_out is None else d_out)))

    def vad_viterbi_batch(self, d_scores, frame_off, n_states, word_state, stay, exit_, enter):
        """spkd_vad_viterbi for every file of concatenated device scores in one launch
        (spkd_vad_viterbi_batch) -> (tok_off int64 [n_files + 1], token first frames int64 (relative
        to the file), token words int32, path scores [n_files]); copies: the library's arrays live
        until the next call."""
        off = self._frame_off(frame_off)
        ws = np.ascontiguousarray(word_state, dtype=np.int32)
        consts = [np.ascontiguousarray(a, dtype=np.float64) for a in (stay, exit_, enter)]
        if any(len(a) != len(ws) for a in consts):
            raise SpkdError(SPKD_EINVAL, 'one constant of each kind per word')
        n = len(off) - 1
        out = [C.c_void_p() for _ in range(4)]
        self.check(self.lib.spkd_vad_viterbi_batch(self.h, C.c_void_p(d_scores), n, _ptr(off), int(n_states), len(ws),
                                                   _ptr(ws), *[_ptr(a) for a in consts], *[C.byref(o) for o in out]))
        return self._tokens(out, n)

    # ---- (8) resegmentation
    def gauss_models(self, d_stats, n, d_models):
        """One full-covariance Gaussian model (GAUSS_MODEL doubles: mu, W = L^-1 packed, c) per
        statistics record of d_stats into d_models (spkd_gauss_models).  Returns ok (int32 [n]):
        0 for a record that cannot be modelled (fewer than 40 frames, no positive pivot, not
        finite), whose model may hold anything.  The kernel's time is last_ms('gauss_models')."""
        ok = np.zeros(int(n), dtype=np.int32)
        self.check(self.lib.spkd_gauss_models(self.h, C.c_void_p(d_stats), int(n), C.c_void_p(d_models), _ptr(ok)))
        return ok

    def gauss_loglik(self, d_frames, n_frames, d_models, model_ok, seq_begin, seq_end, seq_model, seq_n_models,
                     n_cols, d_scores):
        """The log-likelihood of every frame of the sequences [seq_begin[q], seq_end[q]) under the
        models seq_model[q] .. + seq_n_models[q] - 1 (spkd_gauss_loglik) into the compact device
        array d_scores [sum len, n_cols] float32; -inf in the columns of models that are not ok and
        from seq_n_models[q] on.  Returns frame_off, the running sum of the lengths: what
        vad_viterbi_batch takes with these scores.  The kernel's time is last_ms('gauss_loglik')."""
        seqs, frame_off = self._seq_args(model_ok, seq_begin, seq_end, seq_model, seq_n_models)
        self.check(self.lib.spkd_gauss_loglik(self.h, C.c_void_p(d_frames), int(n_frames), C.c_void_p(d_models), *seqs,
                                              int(n_cols), C.c_void_p(d_scores)))
        return frame_off

    def mindur_viterbi_batch(self, d_scores, frame_off, n_cols, penalty, min_frames):
        """The speaker loop with a minimum duration for every sequence of concatenated device scores
        [sum T, n_cols] in one launch (spkd_mindur_viterbi_batch): word k is column k, entering a word
        costs `penalty`, no stretch is shorter than min_frames frames unless it is a whole sequence.
        Returns what vad_viterbi_batch returns: (tok_off, token first frames, token words, path
        scores); copies.  The kernels' times are last_ms('mindur_viterbi') and last_ms('mindur_backtrack')."""
        off = self._frame_off(frame_off)
        n = len(off) - 1
        out = [C.c_void_p() for _ in range(4)]
        self.check(self.lib.spkd_mindur_viterbi_batch(self.h, C.c_void_p(d_scores), n, _ptr(off), int(n_cols), float(penalty),
                                                      int(min_frames), *[C.byref(o) for o in out]))
        return self._tokens(out, n)

    def fb_posterior_batch(self, d_scores, frame_off, n_cols, penalty, tokens=None, seq_n_cols=None, scale=1.0, d_post=0):
        """The posteriors of the speaker loop (stay 0, switch -penalty) on every sequence of concatenated
        device scores [sum T, n_cols] in one launch (spkd_fb_posterior_batch).  tokens: (tok_off, token
        first frames, token words) as a decoder returns them, or None; seq_n_cols: the columns each
        sequence uses (None: n_cols); scale: the acoustic scale, scale * penalty <= 600; d_post: 0 or a
        device array [sum T, n_cols] float32 that receives every frame's posteriors.  Returns (conf,
        logz): per token the mean posterior of its word over its frames (None without tokens) and per
        sequence the log-evidence.  The kernel's time is last_ms('fb_posterior')."""
        off = self._frame_off(frame_off)
        n = len(off) - 1
        c = np.ascontiguousarray
        ncol = None
        if seq_n_cols is not None:
            ncol = c(seq_n_cols, dtype=np.int32)
            if ncol.ndim != 1 or len(ncol) != n:
                raise SpkdError(SPKD_EINVAL, 'seq_n_cols: one entry per sequence')
        tok = [None, None, None]
        conf = None
        if tokens is not None:
            tok = [c(tokens[0], dtype=np.int64), c(tokens[1], dtype=np.int64), c(tokens[2], dtype=np.int32)]
            if any(a.ndim != 1 for a in tok) or len(tok[0]) != n + 1 or len(tok[1]) != len(tok[2]) or \
                    int(tok[0].min()) < 0 or int(tok[0].max()) > len(tok[1]):
                raise SpkdError(SPKD_EINVAL, 'tokens: tok_off with one entry per sequence and the total, a frame and a word per token')
            conf = np.zeros(len(tok[1]), dtype=np.float64)
        logz = np.zeros(n, dtype=np.float64)
        p = lambda a: None if a is None else _ptr(a)
        self.check(self.lib.spkd_fb_posterior_batch(self.h, C.c_void_p(d_scores), n, _ptr(off), int(n_cols), float(penalty),
                                                    float(scale), p(ncol), p(tok[0]), p(tok[1]), p(tok[2]),
                                                    C.c_void_p(d_post) if d_post else None, p(conf), _ptr(logz)))
        return conf, logz

    def post_stats(self, d_frames, n_frames, d_post, seq_begin, seq_end, seq_model, seq_n_models, n_cols, n_models, d_stats,
                   masses=True):
        """Posterior-weighted statistics records (spkd_post_stats): record m of d_stats (n_models records
        as set_stats leaves them) is the sum, over every frame of the sequences whose models
        seq_model[q] .. + seq_n_models[q] - 1 include m, of d_post[row, m - seq_model[q]] * [x; 1] [x; 1]^T.
        The sequences and n_cols are gauss_loglik's; d_post is the compact device array [sum len, n_cols]
        float32 in that call's score layout, as fb_posterior_batch writes it.  A weight of exactly 0 adds
        nothing whatever the frame holds; a model no sequence covers gets zeros.  Returns the records'
        count entries, float64 [n_models]: each model's expected number of frames (the records come down
        for it, 6 560 bytes each; masses=False: no copy, None).  The kernels' time is last_ms('post_stats')."""
        c = np.ascontiguousarray
        b, e = c(seq_begin, dtype=np.int64), c(seq_end, dtype=np.int64)
        m, k = c(seq_model, dtype=np.int32), c(seq_n_models, dtype=np.int32)
        if any(a.ndim != 1 for a in (b, e, m, k)) or not (len(b) == len(e) == len(m) == len(k)):
            raise SpkdError(SPKD_EINVAL, 'one begin, end, first model and model count per sequence')
        self.check(self.lib.spkd_post_stats(self.h, C.c_void_p(d_frames), int(n_frames), C.c_void_p(d_post), len(b), _ptr(b),
                                            _ptr(e), _ptr(m), _ptr(k), int(n_cols), int(n_models), C.c_void_p(d_stats)))
        if not masses:
            return None
        rec = np.empty((int(n_models), REC), dtype=np.float64)
        if rec.size:
            self.d2h(rec, d_stats)
        return rec[:, REC - 1].copy()

    # ---- (9) resegmentation with mixture models
    def gmm_train(self, d_frames, n_frames, set_off, range_begin, range_end, n_comp, n_iter, var_floor, d_gmm,
                  from_model=False):
        """One diagonal-covariance mixture of n_comp components (GMM_COMP doubles each: ln w, mean,
        1 / var, log_norm) per speaker into d_gmm, trained by n_iter EM steps on the device
        (spkd_gmm_train): speaker s owns the frame ranges set_off[s] .. set_off[s + 1] of range_begin /
        range_end, in that order.  from_model: start from what d_gmm holds instead of the segmental
        initial model.  Returns (ok int32 [n_speakers], loglik [n_speakers, n_iter]): ok 0 for a
        speaker that cannot be modelled (fewer than 40 n_comp frames, constant or non-finite frames),
        loglik[s, i] the total log-likelihood of speaker s's frames under the model that entered
        iteration i.  The time of all its kernels is last_ms('gmm_train')."""
        sets = self._range_sets(set_off, range_begin, range_end)
        ok = np.zeros(sets[0], dtype=np.int32)
        ll = np.zeros((sets[0], max(int(n_iter), 0)), dtype=np.float64)
        self.check(self.lib.spkd_gmm_train(self.h, C.c_void_p(d_frames), int(n_frames), *sets, int(n_comp), int(n_iter),
                                           1 if from_model else 0, float(var_floor), C.c_void_p(d_gmm), _ptr(ok),
                                           _ptr(ll) if ll.size else None))
        return ok, ll

    def gmm_loglik_seq(self, d_frames, n_frames, d_gmm, n_comp, model_ok, seq_begin, seq_end, seq_model, seq_n_models,
                       n_cols, d_scores):
        """gauss_loglik under mixtures (spkd_gmm_loglik_seq): d_gmm holds len(model_ok) models of n_comp
        components as gmm_train leaves them, model_ok its ok.  Returns frame_off.  The kernel's time
        is last_ms('gmm_seq_loglik')."""
        seqs, frame_off = self._seq_args(model_ok, seq_begin, seq_end, seq_model, seq_n_models)
        self.check(self.lib.spkd_gmm_loglik_seq(self.h, C.c_void_p(d_frames), int(n_frames), C.c_void_p(d_gmm), int(n_comp),
                                                *seqs, int(n_cols), C.c_void_p(d_scores)))
        return frame_off

    # ---- (10) linking by cross-likelihood ratio
    def ubm_stats(self, d_frames, n_frames, d_ubm, n_comp, set_off, range_begin, range_end, d_bw):
        """The record of every speaker under the one UBM at d_ubm (n_comp components as gmm_train leaves
        them) into d_bw: BW_COMP doubles a component, n_c = sum g_c and f_c = sum g_c x over the
        speaker's frames (spkd_ubm_stats).  The speakers own their ranges as in gmm_train.  Returns ok
        int32 [n_speakers]: 0 for a speaker without a frame or with a sum that is not finite.  The
        kernels' time is last_ms('ubm_stats')."""
        sets = self._range_sets(set_off, range_begin, range_end)
        ok = np.zeros(sets[0], dtype=np.int32)
        self.check(self.lib.spkd_ubm_stats(self.h, C.c_void_p(d_frames), int(n_frames), C.c_void_p(d_ubm), int(n_comp),
                                           *sets, C.c_void_p(d_bw), _ptr(ok)))
        return ok

    def feature_warp(self, d_frames, n_frames, set_off, range_begin, range_end, window, d_out):
        """Feature warping of the frames at d_frames into d_out (spkd_feature_warp; the rule is
        include/spkd.h, section 10b): set s -- one file's speech -- owns the frame ranges set_off[s] ..
        set_off[s + 1] of range_begin / range_end, ascending and disjoint over the whole list; within a set
        every coefficient becomes the standard-normal quantile of its rank among the `window` compacted
        frames around it.  The quantile tables (warp_table) are built here, one per distinct
        min(window, frames of a set), and kept by the context.  A frame in no range is not written.  The
        kernel's time is last_ms('feature_warp')."""
        n_sets, p_off, p_b, p_e = self._range_sets(set_off, range_begin, range_end)
        off, b, e = (np.asarray(a, dtype=np.int64) for a in (set_off, range_begin, range_end))
        length = np.zeros(n_sets, dtype=np.int64)
        owner = np.repeat(np.arange(n_sets), np.maximum(np.diff(off), 0))
        if len(owner) == len(b):                 # (offsets that go back: the library refuses them, no table is needed)
            np.add.at(length, owner, e - b)
        cache = self.__dict__.setdefault('_warp_tables', {})
        table, at, table_off = [], {}, np.zeros(n_sets, dtype=np.int64)
        for s, n in enumerate(np.clip(length, 0, max(int(window), 0)).tolist()):
            if n < 1:
                continue
            if n not in at:
                if n not in cache:
                    cache[n] = warp_table(n)
                at[n] = sum(len(t) for t in table)
                table.append(cache[n])
            table_off[s] = at[n]
        table = np.ascontiguousarray(np.concatenate(table + [np.zeros(1, dtype=np.float32)]))
        self.check(self.lib.spkd_feature_warp(self.h, C.c_void_p(d_frames), int(n_frames), n_sets, p_off, p_b, p_e, int(window),
                                              _ptr(table), len(table), _ptr(table_off), C.c_void_p(d_out)))

    def clr_link(self, d_bw, ok, d_ubm, n_comp, relevance, threshold, max_spk=0):
        """The agglomerative chain over the len(ok) records at d_bw by cross-likelihood ratio under
        means MAP-adapted from the UBM (spkd_clr_link), in one call.  Returns dict(status, n_merges, a,
        b, d, stat_max, stat_min): the merge log in spkd_ahc's convention (labels_from_merges replays
        it); status is SPKD_ENONFINITE, with the log so far, when a ratio among ok speakers was not
        finite.  The kernels' time is last_ms('clr_link')."""
        ok = np.ascontiguousarray(ok, dtype=np.int32)
        if ok.ndim != 1:
            raise SpkdError(SPKD_EINVAL, 'ok: one flag per record')
        n = len(ok)
        ma, mb, md = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64)
        nm = np.zeros(1, dtype=np.int32)
        smax, smin = np.full(1, np.nan), np.full(1, np.nan)
        st = self.lib.spkd_clr_link(self.h, C.c_void_p(d_bw), n, _ptr(ok), C.c_void_p(d_ubm), int(n_comp), float(relevance),
                                    float(threshold), int(max_spk), _ptr(ma), _ptr(mb), _ptr(md), _ptr(nm), _ptr(smax),
                                    _ptr(smin))
        self.check(st, allow=(SPKD_ENONFINITE,))
        k = int(nm[0])
        return dict(status=st, n_merges=k, a=ma[:k], b=mb[:k], d=md[:k], stat_max=float(smax[0]), stat_min=float(smin[0]))

    # ---- (11) a gallery of enrolled speakers
    def clr_identify(self, d_probe_bw, probe_ok, group_off, d_gallery_bw, gallery_ok, d_ubm, n_comp, relevance,
                     threshold, exclusive=True, d_scores=None):
        """The len(probe_ok) records at d_probe_bw against the len(gallery_ok) records at d_gallery_bw by
        cross-likelihood ratio under the UBM at d_ubm (spkd_clr_identify).  group_off: the probes of
        group k are group_off[k] .. group_off[k + 1]; under `exclusive` the probes of a group get
        distinct identities, by a greedy chain over the scores above `threshold`.  Returns dict(status,
        ident, score, second): ident int32 (-1: unknown), score the assigned pair's or an unknown
        probe's highest, second the highest over the other identities (NaN: none).  status is
        SPKD_ENONFINITE, with every ident -1, when a score among ok records was not finite.  d_scores:
        a device buffer of len(probe_ok) * len(gallery_ok) doubles that receives the matrix.  The
        kernels' times are last_ms('ident_scores') and last_ms('ident_assign')."""
        pok = np.ascontiguousarray(probe_ok, dtype=np.int32)
        gok = np.ascontiguousarray(gallery_ok, dtype=np.int32)
        off = np.ascontiguousarray(group_off, dtype=np.int64)
        if pok.ndim != 1 or gok.ndim != 1 or off.ndim != 1 or len(off) < 1:
            raise SpkdError(SPKD_EINVAL, 'ok: one flag per record; group_off: one offset per group and the end')
        n = len(pok)
        ident = np.full(n, -1, dtype=np.int32)
        score, second = np.full(n, np.nan), np.full(n, np.nan)
        st = self.lib.spkd_clr_identify(self.h, C.c_void_p(d_probe_bw), n, _ptr(pok), len(off) - 1, _ptr(off),
                                        C.c_void_p(d_gallery_bw), len(gok), _ptr(gok), C.c_void_p(d_ubm), int(n_comp),
                                        float(relevance), float(threshold), 1 if exclusive else 0, _ptr(ident),
                                        _ptr(score), _ptr(second), C.c_void_p(d_scores) if d_scores else None)
        self.check(st, allow=(SPKD_ENONFINITE,))
        return dict(status=st, ident=ident, score=score, second=second)

    def bw_accumulate(self, d_src_bw, n_src, n_comp, set_off, member, dst, keep, d_dst_bw, n_dst):
        """dst[dst[k]] = (keep[k] ? dst[dst[k]] : 0) + the records member[set_off[k]:set_off[k + 1]] of
        d_src_bw, in that order (spkd_bw_accumulate): the sum of a cluster's records, or a record added
        to its identity.  The kernel's time is last_ms('bw_accumulate')."""
        off = np.ascontiguousarray(set_off, dtype=np.int64)
        mem = np.ascontiguousarray(member, dtype=np.int32)
        slot = np.ascontiguousarray(dst, dtype=np.int32)
        kp = np.ascontiguousarray(keep, dtype=np.int32)
        if off.ndim != 1 or len(off) < 1 or len(slot) != len(off) - 1 or len(kp) != len(slot) or len(mem) != int(off[-1]):
            raise SpkdError(SPKD_EINVAL, 'bw_accumulate: one slot and one keep flag per set, set_off[-1] members')
        self.check(self.lib.spkd_bw_accumulate(self.h, C.c_void_p(d_src_bw), int(n_src), int(n_comp), len(slot), _ptr(off),
                                               _ptr(mem), _ptr(slot), _ptr(kp), C.c_void_p(d_dst_bw), int(n_dst)))

    # ---- (4)
    def ahc(self, d_stats, seg_off, params):
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        npb = len(seg_off) - 1
        nt = int(seg_off[-1])
        n_merges = np.zeros(npb, dtype=np.int32)
        ma = np.zeros(nt, dtype=np.int32)
        mb = np.zeros(nt, dtype=np.int32)
        md = np.zeros(nt, dtype=np.float64)
        smax = np.zeros(npb, dtype=np.float64)
        smin = np.zeros(npb, dtype=np.float64)
        st = self.lib.spkd_ahc(self.h, C.c_void_p(d_stats), _ptr(seg_off), npb, C.byref(params),
                               _ptr(n_merges), _ptr(ma), _ptr(mb), _ptr(md), _ptr(smax), _ptr(smin))
        self.check(st, allow=(SPKD_ENONFINITE,))
        return dict(status=st, n_merges=n_merges, a=ma, b=mb, d=md, stat_max=smax, stat_min=smin)

    def distance_rows(self, variant, kind, lambdac, d_stats, n, row_begin, row_end, d_rows):
        """Rows [row_begin, row_end) of the initial matrix of one n-record problem -> d_rows
        (device, (row_end - row_begin) * n doubles); returns (max, min) over the block's finite
        distances (NaN: none)."""
        smax, smin = C.c_double(), C.c_double()
        st = self.lib.spkd_distance_rows(self.h, int(variant), KINDS[kind] if isinstance(kind, str) else int(kind),
                                         float(lambdac), C.c_void_p(d_stats), int(n), int(row_begin), int(row_end),
                                         C.c_void_p(d_rows), C.byref(smax), C.byref(smin))
        self.check(st, allow=(SPKD_ENONFINITE,))
        if st == SPKD_ENONFINITE:
            raise ValueError('array must not contain infs or NaNs')
        return smax.value, smin.value

    def cluster_in(self, d_stats, n, kind, lambdac, threshold):
        """spk_cluster_in over n records in recipe order as one device chain -> (labels[n],
        per-record distance lists (done records only), records done, clusters, status).  status is
        SPKD_ENONFINITE when a covariance with infs or NaNs stopped the chain at record `done`."""
        n = int(n)
        label = np.zeros(max(n, 1), dtype=np.int32)
        off = np.zeros(n + 1, dtype=np.int64)
        done, nclu = C.c_int64(0), C.c_int64(0)
        full = n * (n - 1) // 2
        cap = min(full, 32 * n)
        while True:
            dist = np.empty(max(cap, 1), dtype=np.float64)
            st = self.lib.spkd_cluster_in(self.h, C.c_void_p(d_stats), n, KINDS[kind] if isinstance(kind, str) else int(kind),
                                          float(lambdac), float(threshold), _ptr(label), _ptr(dist), cap, _ptr(off),
                                          C.byref(done), C.byref(nclu))
            if st == SPKD_EOVERFLOW and cap < full:
                cap = min(full, 4 * cap)
                continue
            break
        self.check(st, allow=(SPKD_ENONFINITE,))
        nd = int(done.value)
        dists = [dist[int(off[s]):int(off[s + 1])].copy() for s in range(nd)]
        return label[:n], dists, nd, int(nclu.value), st

    def cluster_in_batch(self, d_stats, seg_off, kind, lambdac, threshold):
        """spk_cluster_in for every problem of seg_off in one launch (spkd_cluster_in_batch), each
        as cluster_in on its records alone -> dict: label (0-based within the problem) and mind
        per record, n_done, n_clusters, stat_max, stat_min per problem, status.  status is
        SPKD_ENONFINITE when a covariance with infs or NaNs stopped a problem (n_done[p] < its
        size); the other problems are complete."""
        seg_off = np.ascontiguousarray(seg_off, dtype=np.int64)
        if seg_off.ndim != 1 or len(seg_off) < 1:
            raise SpkdError(SPKD_EINVAL, 'seg_off: one entry per problem and the total')
        npb = len(seg_off) - 1
        nt = max(int(seg_off[-1]), 0)
        label = np.zeros(nt, dtype=np.int32)
        mind = np.zeros(nt, dtype=np.float64)
        done = np.zeros(npb, dtype=np.int64)
        nclu = np.zeros(npb, dtype=np.int64)
        smax = np.full(npb, np.nan)
        smin = np.full(npb, np.nan)
        st = self.lib.spkd_cluster_in_batch(self.h, C.c_void_p(d_stats), npb, _ptr(seg_off),
                                            KINDS[kind] if isinstance(kind, str) else int(kind), float(lambdac),
                                            float(threshold), _ptr(label), _ptr(mind), _ptr(done), _ptr(nclu),
                                            _ptr(smax), _ptr(smin))
        self.check(st, allow=(SPKD_ENONFINITE,))
        return dict(status=st, label=label, mind=mind, n_done=done, n_clusters=nclu, stat_max=smax, stat_min=smin)

    def ahc_matrix(self, d_stats, n, params, d_matrix, stat_max_in=float('nan'), stat_min_in=float('nan')):
        """The merge loop of one n-record problem on a caller-supplied initial matrix."""
        n = int(n)
        n_merges = np.zeros(1, dtype=np.int32)
        ma = np.zeros(n, dtype=np.int32)
        mb = np.zeros(n, dtype=np.int32)
        md = np.zeros(n, dtype=np.float64)
        smax = np.zeros(1, dtype=np.float64)
        smin = np.zeros(1, dtype=np.float64)
        st = self.lib.spkd_ahc_matrix(self.h, C.c_void_p(d_stats), n, C.byref(params), C.c_void_p(d_matrix),
                                      float(stat_max_in), float(stat_min_in), _ptr(n_merges), _ptr(ma), _ptr(mb),
                                      _ptr(md), _ptr(smax), _ptr(smin))
        self.check(st, allow=(SPKD_ENONFINITE,))
        return dict(status=st, n_merges=n_merges, a=ma, b=mb, d=md, stat_max=smax, stat_min=smin)
