"""ctypes binding of libbvc.so (include/bvc.h).  Device memory, streams and multi-process plumbing come
from torch; the arithmetic is all inside the library's HIP kernels."""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("BVC_LIBBVC") or os.path.join(_HERE, "libbvc.so")      # (BVC_LIBBVC: a variant build for A/B runs, tools/)

BVC_PTR_HOST = 0
BVC_PTR_DEVICE = 1
NCLASS = 512


class BvcError(RuntimeError):
    """status: the library's return code (BVC_ERR_*, include/bvc.h) where the error came from a call, else None."""
    status = None


class SiteResult(C.Structure):          # bvc_site_result, 120 bytes
    _fields_ = [
        ("var_qual", C.c_double), ("chi", C.c_double), ("depth_total", C.c_double),
        ("af", C.c_double * 3), ("lr_alt", C.c_double), ("base_frq", C.c_double * 4),
        ("depth", C.c_int32 * 4), ("n_passes", C.c_int32), ("alt_base", C.c_int8 * 3),
        ("n_alt", C.c_uint8), ("called", C.c_uint8), ("n_kept", C.c_uint8), ("kept", C.c_int8 * 4),
        ("status", C.c_uint8), ("n_fits", C.c_uint8),
    ]


class GroupResult(C.Structure):         # bvc_group_result, 48 bytes
    _fields_ = [("af", C.c_double * 3), ("depth", C.c_int32 * 4), ("ran", C.c_uint8), ("present", C.c_uint8),
                ("pad", C.c_uint8 * 6)]


class Profile(C.Structure):
    _fields_ = [("hist_ms", C.c_double), ("em_ms", C.c_double), ("hist_launches", C.c_int64),
                ("em_launches", C.c_int64), ("sites", C.c_int64)]


SITE_DTYPE = np.dtype(SiteResult)
GROUP_DTYPE = np.dtype(GroupResult)
# bvc_site_stats, 64 bytes: the called sites' rank sums (rank2 = 2 x rankR1 of the REF observations: mapq, qual, rpr) and strand counts
STATS_DTYPE = np.dtype([("rank2", "<i8", (3,)), ("n_ref", "<i4"), ("n_alt", "<i4"), ("ref_fwd", "<i4"), ("ref_rev", "<i4"),
                        ("alt_fwd", "<i4"), ("alt_rev", "<i4"), ("valid", "u1"), ("pad", "u1", (15,))])
ENTRY_DTYPE = np.dtype([("base", "u1"), ("mapq", "u1"), ("qual", "u1"), ("rpr", "u1"), ("strand", "u1"), ("is_indel", "u1"), ("pad", "<u2")])
TALLY_DTYPE = np.dtype([("strand_base", "<u4", (8,)), ("n_other", "<u4"), ("n_indel", "<u4"), ("pad", "<u4", (2,))])            # bvc_bam_site_tally
INDEL_DTYPE = np.dtype([("entry", "<i8"), ("text_off", "<i8"), ("len", "<i4"), ("pad", "<i4")])                 # bvc_pileup_indel
BLOCK_DTYPE = np.dtype([("comp_off", "<i8"), ("out_off", "<i8"), ("comp_len", "<i4"), ("isize", "<i4"), ("crc32", "<u4"),
                        ("check_crc", "<u4")])                                                                   # bvc_bgzf_block
SITE_STATS_TRIP = 4096      # entries a workgroup of site_stats_kernel takes per trip of its loop (csrc/bvc_internal.h, kSiteStatsTrip)
VCF_SAMPLES_TILE = 508      # samples a workgroup of vcf_samples_kernel formats per trip of its loop (csrc/bvc_internal.h, kVcfSamplesTile)
assert SITE_DTYPE.itemsize == C.sizeof(SiteResult) == 120
assert STATS_DTYPE.itemsize == 64 and ENTRY_DTYPE.itemsize == 8 and TALLY_DTYPE.itemsize == 48
assert GROUP_DTYPE.itemsize == C.sizeof(GroupResult) == 48

# The C ABI, one row per function: name -> (restype, argtypes), in the order of include/bvc.h (tests/test_binding_abi.py compares
# the two).  A new entry point takes a row here and a Context method below.
_vp, _i64, _i32, _u32, _dbl, _int = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_double, C.c_int
_pi64 = C.POINTER(C.c_int64)
PROTOTYPES = {
    "bvc_version": (C.c_char_p, []),
    "bvc_device_count": (_int, []),
    "bvc_create": (_int, [C.POINTER(_vp), _int]),
    "bvc_destroy": (None, [_vp]),
    "bvc_host_alloc": (_vp, [C.c_size_t]),
    "bvc_host_free": (None, [_vp]),
    "bvc_last_error": (C.c_char_p, [_vp]),
    "bvc_set_stream": (_int, [_vp, _vp]),
    "bvc_synchronize": (_int, [_vp]),
    "bvc_set_overlap": (_int, [_vp, _int]),
    "bvc_join": (_int, [_vp]),
    "bvc_set_profiling": (_int, [_vp, _int]),
    "bvc_get_profile": (_int, [_vp, C.POINTER(Profile), _int]),
    "bvc_lrt_dense": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _dbl, _vp, _u32]),
    "bvc_lrt_dense_groups": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _dbl, _vp, _i32, _vp, _vp, _u32]),
    "bvc_lrt_csr": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _dbl, _vp, _u32]),
    "bvc_lrt_csr_comb": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _dbl, _vp, _vp, _vp, _u32]),
    "bvc_lrt_csr_packed": (_int, [_vp, _i64, _vp, _vp, _vp, _dbl, _vp, _u32]),
    "bvc_lrt_dense_packed": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _dbl, _vp, _u32]),
    "bvc_lrt_dense_groups_packed": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _dbl, _vp, _i32, _vp, _vp, _u32]),
    "bvc_pack_dense": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _pi64, _u32]),
    "bvc_lrt_csr_groups": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _vp, _i64, _i32, _vp, _vp, _u32]),
    "bvc_lrt_csr_group_labels": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _dbl, _i32, _vp, _vp, _u32]),
    "bvc_lrt_csr_group_labels_packed": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _dbl, _i32, _vp, _vp, _u32]),
    "bvc_inflate_blocks": (_int, [_vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _u32]),
    "bvc_pileup_begin": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _pi64, _pi64]),
    "bvc_pileup_finish": (_int, [_vp, _vp, _dbl, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bvc_pileup_begin_bin": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _pi64, _pi64]),
    "bvc_pileup_finish_called": (_int, [_vp, _vp, _dbl, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bvc_site_stats_csr": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _u32]),
    "bvc_pileup_finish_called_stats": (_int, [_vp, _vp, _dbl, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                              _vp, _vp]),
    "bvc_pileup_begin_bgzf": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, C.POINTER(_i32), _vp, _pi64, _pi64, _pi64]),
    "bvc_pileup_text": (_int, [_vp, _vp, _i64, _pi64, _vp]),
    "bvc_hist_dense": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _u32]),
    "bvc_hist_dense_packed": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _u32]),
    "bvc_lrt_hist": (_int, [_vp, _i64, _vp, _vp, _dbl, _vp, _vp, _vp, _u32]),
    "bvc_counts_add_dense": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _u32]),
    "bvc_counts_add_dense_packed": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _u32]),
    "bvc_counts_add_csr": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _u32]),
    "bvc_counts_add_csr_packed": (_int, [_vp, _i64, _vp, _vp, _vp, _u32]),
    "bvc_counts_add_dense_groups": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _i32, _vp, _u32]),
    "bvc_counts_add_csr_group_labels": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _u32]),
    "bvc_lrt_hist_groups": (_int, [_vp, _i64, _vp, _vp, _dbl, _i32, _vp, _vp, _u32]),
    "bvc_counts_merge": (_int, [_vp, _i64, _vp, _vp, _u32]),
    "bvc_synth_dense": (_int, [_vp, C.c_uint64, _i64, _i64, _i64, _i64, _u32, _vp, _vp, _vp]),
    "bvc_set_tuning": (_int, [_vp, C.c_char_p, _int]),
    "bvc_stream_read_ms": (_int, [_vp, _vp, _i64, _int, C.POINTER(_dbl)]),
    "bvc_vcf_bp_lut": (None, [_vp]),
    "bvc_vcf_samples_csr": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _u32]),
    "bvc_pileup_finish_called_text": (_int, [_vp, _vp, _dbl, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "bvc_pileup_sample_text": (_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "bvc_bgzf_deflate": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _u32]),
    "bvc_pileup_sample_bgzf": (_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    # not in the header: diagnostic builds of the library only export it (-DBVC_CHECK_LDS, csrc/bvc_device.h)
    "bvc_debug_report": (_int, [_vp, C.POINTER(_u32), _int]),
}
# The second header, include/bvc_bgzf_codes.h: the same kind of table, in that header's order (tests/test_bgzf_dynamic_abi.py compares
# the two as tests/test_binding_abi.py compares the first with bvc.h), bound by bind() with the first.
BGZF_CODES_PROTOTYPES = {
    "bvc_bgzf_code_lengths": (_int, [_vp, _i64, _vp, _i32, _i32, _vp]),
}
BGZF_CODES_EXPORTS = list(BGZF_CODES_PROTOTYPES)
# The third header, include/bvc_bam.h (tests/test_bam_pileup_abi.py compares the two), bound by bind() with the others.
BAM_PROTOTYPES = {
    "bvc_bam_pileup": (_int, [_vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _pi64, _vp, _vp, _u32]),
    "bvc_bam_pileup_bgzf": (_int, [_vp, _i32, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp, _i64,
                                   _pi64, _vp, _vp]),
}
BAM_EXPORTS = list(BAM_PROTOTYPES)
# The fourth header, include/bvc_popmatrix.h (tests/test_popmatrix_abi.py compares the two), bound by bind() with the others.
POPMATRIX_PROTOTYPES = {
    "bvc_bam_popmatrix": (_int, [_vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _vp, _u32]),
    "bvc_bam_popmatrix_bgzf": (_int, [_vp, _i32, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i64, _vp,
                                      _i64, _vp]),
}
POPMATRIX_EXPORTS = list(POPMATRIX_PROTOTYPES)
# The fifth header, include/bvc_bam_text.h (tests/test_bam_text_abi.py compares the two), bound by bind() with the others: the twins of
# BAM_PROTOTYPES' calls for the text temp batches, argument for argument.
BAM_TEXT_PROTOTYPES = {
    "bvc_bam_pileup_text": BAM_PROTOTYPES["bvc_bam_pileup"],
    "bvc_bam_pileup_text_bgzf": BAM_PROTOTYPES["bvc_bam_pileup_bgzf"],
}
BAM_TEXT_EXPORTS = list(BAM_TEXT_PROTOTYPES)
# The sixth header, include/bvc_store.h (tests/test_store_abi.py compares the two), bound by bind() with the others: temp batches kept on
# the device.  bvc_bam_pileup_bgzf_store takes bvc_bam_pileup_bgzf's arguments up to refseq_len, then the store and the batch's index.
STORE_PROTOTYPES = {
    "bvc_store_create": (_int, [C.POINTER(_vp), _int, _i32, _i32, _i64]),
    "bvc_store_destroy": (None, [_vp]),
    "bvc_store_put": (_int, [_vp, _vp, _i32, _i32, _vp, _i64, _vp]),
    "bvc_bam_pileup_bgzf_store": (_int, BAM_PROTOTYPES["bvc_bam_pileup_bgzf"][1][:19] + [_vp, _i32, _pi64, _vp]),
    "bvc_store_get": (_int, [_vp, _vp, _i32, _vp, _i64, _pi64, _vp]),
    "bvc_store_seal": (_int, [_vp, _vp]),
    "bvc_store_tile": (_int, [_vp, _i32, _i32, _i64, C.POINTER(_i32), _pi64]),
    "bvc_store_bytes": (_int, [_vp, _pi64, _pi64]),
    "bvc_pileup_begin_store": (_int, [_vp, _vp, _i32, _i32, _pi64, _pi64, _pi64]),
}
STORE_EXPORTS = list(STORE_PROTOTYPES)
# The seventh header, include/bvc_bam_deflate.h (tests/test_bam_deflate_abi.py compares the two), bound by bind() with the others: phase 1's temp
# batches deflated on the device.  The two calls take bvc_bam_pileup_bgzf's arguments up to refseq_len, then the pieces and the outputs.
BAM_DEFLATE_PROTOTYPES = {
    "bvc_bam_pileup_bgzf_deflate": (_int, BAM_PROTOTYPES["bvc_bam_pileup_bgzf"][1][:19] + [_i32, _vp, _vp, _i64, _pi64, _vp, _vp, _vp]),
    "bvc_bam_pileup_text_bgzf_deflate": (_int, BAM_PROTOTYPES["bvc_bam_pileup_bgzf"][1][:19] + [_i32, _vp, _vp, _i64, _pi64, _vp, _vp, _vp]),
    "bvc_bam_pileup_deflate_fetch": (_int, [_vp, _vp, _i64]),
}
BAM_DEFLATE_EXPORTS = list(BAM_DEFLATE_PROTOTYPES)
# The eighth header, include/bvc_bam_counts.h (tests/test_bam_counts_abi.py compares the two), bound by bind() with the others: phase 1 added
# straight into class counts.  bvc_bam_counts takes bvc_bam_pileup's arguments up to rg_s, bvc_bam_counts_bgzf_acc bvc_bam_pileup_bgzf's.
BAM_COUNTS_PROTOTYPES = {
    "bvc_bam_counts": (_int, BAM_PROTOTYPES["bvc_bam_pileup"][1][:14] + [_i64, _vp, _i32, _vp, _vp, _vp, _u32]),
    "bvc_site_acc_create": (_int, [C.POINTER(_vp), _int, _i32, _i32, _i64]),
    "bvc_site_acc_destroy": (None, [_vp]),
    "bvc_site_acc_bytes": (_int, [_vp, _pi64, _pi64]),
    "bvc_bam_counts_bgzf_acc": (_int, BAM_PROTOTYPES["bvc_bam_pileup_bgzf"][1][:17] + [_i64, _vp, _vp, _vp]),
    "bvc_site_acc_get": (_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "bvc_site_acc_lrt": (_int, [_vp, _vp, _i32, _i32, _vp, _dbl, _vp, _vp]),
}
BAM_COUNTS_EXPORTS = list(BAM_COUNTS_PROTOTYPES)
# The ninth header, include/bvc_bam_group_depth.h (tests/test_bam_group_depth_abi.py compares the two), bound by bind() with the others: phase 1
# added into one slot of class counts with the groups' depths beside it.  bvc_bam_counts_depth takes bvc_bam_counts's arguments up to tally,
# then group_depth.
BAM_GROUP_DEPTH_PROTOTYPES = {
    "bvc_bam_counts_depth": (_int, BAM_COUNTS_PROTOTYPES["bvc_bam_counts"][1][:19] + [_vp, _vp, _u32]),
    "bvc_site_acc_create_depth": (_int, [C.POINTER(_vp), _int, _i32, _i32, _i64]),
    "bvc_site_acc_get_depth": (_int, [_vp, _vp, _i32, _i32, _vp]),
}
BAM_GROUP_DEPTH_EXPORTS = list(BAM_GROUP_DEPTH_PROTOTYPES)
# The tenth header, include/bvc_site_acc_quals.h (tests/test_bam_counts_quals_abi.py compares the two), bound by bind() with the others: phase 1
# added into narrow rows of class counts [position][4][n_quals].  bvc_bam_counts_quals takes bvc_bam_counts_depth's arguments with n_quals
# behind n_groups.
SITE_ACC_QUALS_PROTOTYPES = {
    "bvc_bam_counts_quals": (_int, BAM_COUNTS_PROTOTYPES["bvc_bam_counts"][1][:17] + [_i32, _vp, _vp, _vp, _vp, _u32]),
    "bvc_site_acc_create_quals": (_int, [C.POINTER(_vp), _int, _i32, _i32, _i32, _i64]),
    "bvc_site_acc_quals": (_int, [_vp, C.POINTER(_i32)]),
}
SITE_ACC_QUALS_EXPORTS = list(SITE_ACC_QUALS_PROTOTYPES)
# The eleventh header, include/bvc_site_acc_pack.h (tests/test_site_acc_pack_abi.py compares the two), bound by bind() with the others: an
# accumulator's rows as the (row_start, cell, count) entries of their non-zero words, and such entries added into an accumulator.
SITE_ACC_PACK_PROTOTYPES = {
    "bvc_site_acc_row_words": (_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "bvc_site_acc_pack": (_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _i64, _pi64, _u32]),
    "bvc_site_acc_add_packed": (_int, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _i64, _u32]),
}
SITE_ACC_PACK_EXPORTS = list(SITE_ACC_PACK_PROTOTYPES)
ACC_MORE = 2                # BVC_ACC_MORE (include/bvc_site_acc_pack.h): bvc_site_acc_pack wants more room for the entries
STORE_CHUNK = 16384         # BVC_STORE_CHUNK (include/bvc_store.h): bytes of a batch's slice one work item of the gather kernel copies
STORE_GRID = 1024           # workgroups of store_gather_kernel at most (csrc/bvc_internal.h, kStoreGrid): more items go round its loop
BAM_MORE = 2                # BVC_BAM_MORE (include/bvc.h): bvc_bam_pileup wants more bytes of a sample, or more room for the records
BGZF_BLOCK_INPUT = 65280    # input bytes of every block of a piece but its last (include/bvc.h, BVC_BGZF_BLOCK_INPUT)
BGZF_DEFLATE_GRID = 256     # workgroups of bgzf_block_kernel (csrc/bvc_internal.h, kBgzfDeflateGrid): more blocks go round its loop
OPTIONAL = ("bvc_debug_report",)                                # bound where the library has them
EXPORTS = [name for name in PROTOTYPES if name not in OPTIONAL]   # what every build of the library exports

_lib = None


def library_path():
    return _LIB


def bind(cdll):
    """Gives every function of PROTOTYPES, BGZF_CODES_PROTOTYPES, BAM_PROTOTYPES, POPMATRIX_PROTOTYPES, BAM_TEXT_PROTOTYPES, STORE_PROTOTYPES,
    BAM_DEFLATE_PROTOTYPES, BAM_COUNTS_PROTOTYPES, BAM_GROUP_DEPTH_PROTOTYPES, SITE_ACC_QUALS_PROTOTYPES and SITE_ACC_PACK_PROTOTYPES its restype / argtypes on `cdll` (libbvc.so or a variant build of it, a ctypes.CDLL).  A required symbol that the library lacks is an AttributeError."""
    for name, (restype, argtypes) in (list(PROTOTYPES.items()) + list(BGZF_CODES_PROTOTYPES.items()) + list(BAM_PROTOTYPES.items()) +
                                      list(POPMATRIX_PROTOTYPES.items()) + list(BAM_TEXT_PROTOTYPES.items()) + list(STORE_PROTOTYPES.items()) +
                                      list(BAM_DEFLATE_PROTOTYPES.items()) + list(BAM_COUNTS_PROTOTYPES.items()) +
                                      list(BAM_GROUP_DEPTH_PROTOTYPES.items()) + list(SITE_ACC_QUALS_PROTOTYPES.items()) +
                                      list(SITE_ACC_PACK_PROTOTYPES.items())):
        if name in OPTIONAL and not hasattr(cdll, name):
            continue
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes
    return cdll


def load_library():
    """Loads libbvc.so.  Raises if it has not been built (there is no fallback implementation)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch is this package's plumbing layer (device memory, streams, torch.distributed) and ships its own
    # HIP runtime.  It must be in the process BEFORE libbvc.so so that libbvc's libamdhip64.so.7 dependency
    # resolves to that same runtime: two HIP runtimes in one process cannot both open the device.
    import torch  # noqa: F401
    if not os.path.exists(_LIB):
        raise BvcError(f"{_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); basevarc_amd has no CPU fallback")
    _lib = bind(C.CDLL(_LIB))
    return _lib


def vcf_samples_slot(n_samples, n_entries):
    """bvc_vcf_samples_slot (include/bvc.h): bytes of a called site's slot in the text of vcf_samples_csr / pileup_sample_text."""
    return (4 * int(n_samples) + 13 * int(n_entries) + 15) // 16 * 16


def vcf_samples_need(n_samples, offsets, results):
    """The sum of the slots: the text buffer vcf_samples_csr / pileup_sample_text need for these sites."""
    o = np.asarray(offsets, dtype=np.int64)
    called = np.asarray(results["called"]) != 0
    return int(sum(vcf_samples_slot(n_samples, n) for n in (o[1:] - o[:-1])[called]))


def bgzf_blocks(length):
    """bvc_bgzf_blocks (include/bvc.h): the BGZF blocks a piece of `length` bytes becomes."""
    return 0 if length <= 0 else (int(length) + BGZF_BLOCK_INPUT - 1) // BGZF_BLOCK_INPUT


def bgzf_bound(length):
    """bvc_bgzf_bound (include/bvc.h): the most bytes the blocks of a piece of `length` bytes take."""
    return 0 if length <= 0 else int(length) + 31 * bgzf_blocks(length)


def vcf_bp_lut():
    """bvc_vcf_bp_lut: the 256 x 8 characters d.dddddd of the BP sub-field, as bytes (no device needed)."""
    out = C.create_string_buffer(2048)
    load_library().bvc_vcf_bp_lut(out)
    return out.raw


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data)


def _dev_ptr(t):
    return C.c_void_p(t.data_ptr())


def _pointers(args, ptr):
    """A call's arguments in the header's order: arrays and tensors become pointers; None (NULL), numbers and ctypes objects pass as they are."""
    return [ptr(a) if isinstance(a, np.ndarray) or hasattr(a, "data_ptr") else a for a in args]


def _as(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _tile(bases_t, quals_t=None):
    """(n_sites, n_samples, row_stride) of a device tile: rows contiguous, and with two tensors both of one stride."""
    assert bases_t.stride(1) == 1 and (quals_t is None or (quals_t.stride(1) == 1 and quals_t.stride(0) == bases_t.stride(0)))
    return (*bases_t.shape, bases_t.stride(0))


def _block_table(blocks, consecutive):
    """blocks: [(comp_off, comp_len, isize[, crc32])]; with a CRC it is compared.  consecutive: the outputs lie one after the other
    (out_off), else out_off stays 0.  Returns (BLOCK_DTYPE table of at least one row, the sum of isize)."""
    tab = np.zeros(max(1, len(blocks)), dtype=BLOCK_DTYPE)
    at = 0
    for i, blk in enumerate(blocks):
        co, cl, isz = blk[:3]
        tab[i] = (co, at if consecutive else 0, cl, isz, blk[3] if len(blk) > 3 else 0, 1 if len(blk) > 3 else 0)
        at += isz
    return tab, at


class Context:
    """One bvc_ctx: one gfx950 device + one HIP stream.  Not shared between threads."""

    def __init__(self, device=0, stream=None):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.bvc_create(C.byref(h), int(device))
        if rc != 0:
            raise BvcError(f"bvc_create(device={device}) failed with code {rc}: no usable gfx950 device "
                           "(libbvc has no CPU fallback)")
        self._h = h
        self.device = int(device)
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "_h", None):
            self._L.bvc_destroy(self._h)
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

    def _check(self, rc):
        if rc != 0:
            err = BvcError(f"libbvc error {rc}: {self._L.bvc_last_error(self._h).decode()}")
            err.status = rc
            raise err

    def _call(self, fn, device, args, records=()):
        """fn(ctx, *args, *records, flags), the shape of every compute entry point: `device` picks host (numpy, synchronous) or device
        (torch tensors, asynchronous on the stream) pointers and the flag.  args: the sizes, input arrays and scalars in the header's
        order.  records: (buffer or None, shape, dtype) per result array; a missing one is np.zeros of the dtype on the host, uint8
        bytes on the device of the first input tensor.  Returns the list of record buffers."""
        bufs = []
        for buf, shape, dtype in records:
            if buf is None and device:
                import torch
                on = next(a for a in args if hasattr(a, "data_ptr")).device
                buf = torch.empty(math.prod(shape) * dtype.itemsize, dtype=torch.uint8, device=on)
            elif buf is None:
                buf = np.zeros(shape, dtype=dtype)
            bufs.append(buf)
        self._check(fn(self._h, *_pointers((*args, *bufs), _dev_ptr if device else _np_ptr), BVC_PTR_DEVICE if device else BVC_PTR_HOST))
        return bufs

    # ---- plumbing
    def set_stream(self, stream):
        """stream: a torch.cuda.Stream, a raw hipStream_t integer, or None for the default stream."""
        raw = 0 if stream is None else int(getattr(stream, "cuda_stream", stream))
        self._check(self._L.bvc_set_stream(self._h, C.c_void_p(raw)))

    def synchronize(self):
        self._check(self._L.bvc_synchronize(self._h))

    def set_overlap(self, on=True):
        """Run stage 2 of each device-pointer call under stage 1 of the next; results need join()/synchronize()."""
        self._check(self._L.bvc_set_overlap(self._h, int(bool(on))))

    def join(self):
        self._check(self._L.bvc_join(self._h))

    def set_profiling(self, on=True):
        self._check(self._L.bvc_set_profiling(self._h, int(bool(on))))

    def profile(self, reset=False):
        p = Profile()
        self._check(self._L.bvc_get_profile(self._h, C.byref(p), int(bool(reset))))
        return dict(hist_ms=p.hist_ms, em_ms=p.em_ms, hist_launches=p.hist_launches,
                    em_launches=p.em_launches, sites=p.sites)

    def debug_report(self, reset=False):
        """Diagnostic builds of the library only (-DBVC_CHECK_LDS, csrc/bvc_device.h): the recorded LDS bound violations as
        {translation unit: [count, check id, value, limit, blockIdx.x, threadIdx.x]}; None with the product library."""
        if not hasattr(self._L, "bvc_debug_report"):
            return None
        out = (C.c_uint32 * 24)()
        self._check(self._L.bvc_debug_report(self._h, out, int(bool(reset))))
        return {tu: [int(x) for x in out[8 * i:8 * i + 6]] for i, tu in enumerate(("hist_kernel", "em_kernel", "em_items"))}

    def set_tuning(self, key, value):
        """Launch policy of this context (include/bvc.h); results never depend on it (but for "em_engine", "em_tiny_regions", "em_prune",
        "bgzf_codes", "bgzf_parse" and "bgzf_cuts", which the header describes)."""
        self._check(self._L.bvc_set_tuning(self._h, key.encode(), int(value)))

    def host_alloc(self, nbytes):
        """bvc_host_alloc: (address, uint8 view of the page-locked bytes); free with host_free(address)."""
        addr = self._L.bvc_host_alloc(int(nbytes))
        if not addr:
            raise BvcError("bvc_host_alloc failed")
        return addr, np.ctypeslib.as_array((C.c_uint8 * int(nbytes)).from_address(addr))

    def host_free(self, addr):
        self._L.bvc_host_free(addr)

    def stream_read_gbs(self, tensor, repeats=5):
        """Empirical HBM read bandwidth (GB/s): a plain 16 B/lane streaming read of `tensor` (device, contiguous)."""
        ms = C.c_double()
        nbytes = tensor.numel() * tensor.element_size()
        self._check(self._L.bvc_stream_read_ms(self._h, _dev_ptr(tensor), nbytes, int(repeats), C.byref(ms)))
        return nbytes / (ms.value * 1e-3) / 1e9

    def synth_dense_device(self, seed, site0, bases_t, quals_t, ref_t, cov_thr16=65536):
        ns, n = bases_t.shape
        self._check(self._L.bvc_synth_dense(self._h, int(seed), int(site0), ns, n, bases_t.stride(0), int(cov_thr16),
                                            _dev_ptr(bases_t), _dev_ptr(quals_t), _dev_ptr(ref_t)))

    # ---- the compute entry points.  Each has one private body (device, sizes, arrays, scalars[, result buffers]) that holds the
    # call's argument list, and two public forms on it: host (numpy in, numpy structured arrays out, synchronous) and *_device
    # (torch tensors on this context's device in, uint8 tensors of the records out, asynchronous on the stream).
    def _lrt_dense(self, device, ns, n, stride, b, q, r, min_af, res=None):
        return self._call(self._L.bvc_lrt_dense, device, (ns, n, stride, b, q, r, float(min_af)), [(res, (ns,), SITE_DTYPE)])[0]

    def lrt_dense(self, bases, quals, ref_base, min_af):
        b, q, r = _as(bases, np.int8), _as(quals, np.int8), _as(ref_base, np.int8)
        if b.ndim != 2 or b.shape != q.shape or r.shape != (b.shape[0],):
            raise ValueError("bases/quals must be [n_sites, n_samples] and ref_base [n_sites]")
        return self._lrt_dense(False, b.shape[0], b.shape[1], b.shape[1], b, q, r, min_af)

    def lrt_dense_device(self, bases_t, quals_t, ref_t, min_af, results_t=None):
        """bases_t/quals_t: int8 [n_sites, row_stride]-strided CUDA tensors; results_t: uint8 [n_sites*120]."""
        return self._lrt_dense(True, *_tile(bases_t, quals_t), bases_t, quals_t, ref_t, min_af, results_t)

    def _lrt_dense_groups(self, device, ns, n, stride, b, q, r, min_af, g, n_groups, res=None, gres=None):
        return tuple(self._call(self._L.bvc_lrt_dense_groups, device, (ns, n, stride, b, q, r, float(min_af), g, int(n_groups)),
                                [(res, (ns,), SITE_DTYPE), (gres, (ns, n_groups), GROUP_DTYPE)]))

    def lrt_dense_groups(self, bases, quals, ref_base, min_af, group_of_sample, n_groups):
        b, q, r, g = _as(bases, np.int8), _as(quals, np.int8), _as(ref_base, np.int8), _as(group_of_sample, np.uint8)
        if b.ndim != 2 or b.shape != q.shape or r.shape != (b.shape[0],) or g.shape != (b.shape[1],):
            raise ValueError("shape mismatch")
        return self._lrt_dense_groups(False, b.shape[0], b.shape[1], b.shape[1], b, q, r, min_af, g, n_groups)

    def lrt_dense_groups_device(self, bases_t, quals_t, ref_t, min_af, group_t, n_groups, results_t=None,
                                grp_results_t=None):
        """Group mode on device tensors; group_t: uint8 [n_samples].  Returns (results_t, grp_results_t)."""
        return self._lrt_dense_groups(True, *_tile(bases_t, quals_t), bases_t, quals_t, ref_t, min_af, group_t, n_groups, results_t, grp_results_t)

    def lrt_csr(self, offsets, bases, quals, ref_base, min_af, base_comb=None, n_comb=None):
        """Ragged sites (the vectors bt_f builds); base_comb/n_comb: optional per-site SetBase lists."""
        o, b, q, r = _as(offsets, np.int64), _as(bases, np.int8), _as(quals, np.int8), _as(ref_base, np.int8)
        n = len(o) - 1
        cb = nc = None
        if base_comb is not None:
            cb = _as(base_comb, np.int8).reshape(-1, 4)
            nc = _as(n_comb, np.uint8)
        return self._call(self._L.bvc_lrt_csr_comb, False, (n, o, b, q, r, float(min_af), cb, nc), [(None, (n,), SITE_DTYPE)])[0]

    def lrt_csr_device(self, offsets_t, bases_t, quals_t, ref_t, min_af, results_t=None):
        """offsets_t: int64 [n_sites + 1]; bases_t/quals_t: int8 [total] CUDA tensors (asynchronous on the stream)."""
        ns = offsets_t.numel() - 1
        return self._call(self._L.bvc_lrt_csr, True, (ns, offsets_t, bases_t, quals_t, ref_t, float(min_af)),
                          [(results_t, (ns,), SITE_DTYPE)])[0]

    def _lrt_csr_packed(self, device, ns, o, pk, r, min_af, res=None):
        return self._call(self._L.bvc_lrt_csr_packed, device, (ns, o, pk, r, float(min_af)), [(res, (ns,), SITE_DTYPE)])[0]

    def lrt_csr_packed(self, offsets, packed, ref_base, min_af):
        """Ragged sites at one byte per observation (base << 6 | qual); host arrays, synchronous."""
        o = _as(offsets, np.int64)
        return self._lrt_csr_packed(False, len(o) - 1, o, _as(packed, np.uint8), _as(ref_base, np.int8), min_af)

    def lrt_csr_packed_device(self, offsets_t, packed_t, ref_t, min_af, results_t=None):
        return self._lrt_csr_packed(True, offsets_t.numel() - 1, offsets_t, packed_t, ref_t, min_af, results_t)

    def _lrt_csr_groups(self, device, ns, o, b, q, sm, r, min_af, g, n_samples, n_groups):
        return tuple(self._call(self._L.bvc_lrt_csr_groups, device, (ns, o, b, q, sm, r, float(min_af), g, n_samples, int(n_groups)),
                                [(None, (ns,), SITE_DTYPE), (None, (ns, n_groups), GROUP_DTYPE)]))

    def lrt_csr_groups(self, offsets, bases, quals, sample_of_obs, ref_base, min_af, group_of_sample, n_groups):
        """The --group loop on ragged sites: per observation its sample index; group_of_sample[n_samples] (>= n_groups: no group)."""
        o, g = _as(offsets, np.int64), _as(group_of_sample, np.uint8)
        return self._lrt_csr_groups(False, len(o) - 1, o, _as(bases, np.int8), _as(quals, np.int8), _as(sample_of_obs, np.int32),
                                    _as(ref_base, np.int8), min_af, g, len(g), n_groups)

    def lrt_csr_groups_device(self, offsets_t, bases_t, quals_t, samples_t, ref_t, min_af, group_t, n_groups):
        return self._lrt_csr_groups(True, offsets_t.numel() - 1, offsets_t, bases_t, quals_t, samples_t, ref_t, min_af, group_t,
                                    group_t.numel(), n_groups)

    def _lrt_csr_group_labels(self, fn, device, ns, columns, g, r, min_af, n_groups):
        """bvc_lrt_csr_group_labels (columns: offsets, bases, quals) and its packed form (offsets, packed)."""
        return tuple(self._call(fn, device, (ns, *columns, g, r, float(min_af), int(n_groups)),
                                [(None, (ns,), SITE_DTYPE), (None, (ns, n_groups), GROUP_DTYPE)]))

    def lrt_csr_group_labels(self, offsets, bases, quals, group_of_obs, ref_base, min_af, n_groups):
        """lrt_csr_groups for a caller who knows each observation's group: one label byte per observation (>= n_groups: no group)."""
        o = _as(offsets, np.int64)
        return self._lrt_csr_group_labels(self._L.bvc_lrt_csr_group_labels, False, len(o) - 1, (o, _as(bases, np.int8), _as(quals, np.int8)),
                                          _as(group_of_obs, np.uint8), _as(ref_base, np.int8), min_af, n_groups)

    def lrt_csr_group_labels_device(self, offsets_t, bases_t, quals_t, group_of_obs_t, ref_t, min_af, n_groups):
        return self._lrt_csr_group_labels(self._L.bvc_lrt_csr_group_labels, True, offsets_t.numel() - 1, (offsets_t, bases_t, quals_t),
                                          group_of_obs_t, ref_t, min_af, n_groups)

    def lrt_csr_group_labels_packed(self, offsets, packed, group_of_obs, ref_base, min_af, n_groups):
        """lrt_csr_group_labels at two bytes per observation: packed = base << 6 | qual (quality bits 63: skipped)."""
        o = _as(offsets, np.int64)
        return self._lrt_csr_group_labels(self._L.bvc_lrt_csr_group_labels_packed, False, len(o) - 1, (o, _as(packed, np.uint8)),
                                          _as(group_of_obs, np.uint8), _as(ref_base, np.int8), min_af, n_groups)

    def lrt_csr_group_labels_packed_device(self, offsets_t, packed_t, group_of_obs_t, ref_t, min_af, n_groups):
        return self._lrt_csr_group_labels(self._L.bvc_lrt_csr_group_labels_packed, True, offsets_t.numel() - 1, (offsets_t, packed_t),
                                          group_of_obs_t, ref_t, min_af, n_groups)

    def _site_stats_csr(self, device, ns, o, e, r, res, stats=None):
        return self._call(self._L.bvc_site_stats_csr, device, (ns, o, e, r, res), [(stats, (ns,), STATS_DTYPE)])[0]

    def site_stats_csr(self, offsets, entries, ref_base, results):
        """bvc_site_stats_csr on host arrays: entries (ENTRY_DTYPE) of site s at offsets[s] .. offsets[s + 1], results (SITE_DTYPE: called,
        n_alt and alt_base are read).  Returns STATS_DTYPE [n_sites]; a site that is not called has an all-zero record."""
        o, e, r, res = _as(offsets, np.int64), _as(entries, ENTRY_DTYPE), _as(ref_base, np.int8), _as(results, SITE_DTYPE)
        n = len(o) - 1
        assert r.shape == (n,) and res.shape == (n,)
        return self._site_stats_csr(False, n, o, e if len(e) else None, r, res)

    def site_stats_csr_device(self, offsets_t, entries_t, ref_t, results_t, stats_t=None):
        """The same on device tensors (entries_t / results_t / the returned tensor: uint8 views of the records); asynchronous on the
        context's stream.  In overlap mode call join() first: the records must be complete."""
        return self._site_stats_csr(True, offsets_t.numel() - 1, offsets_t, entries_t, ref_t, results_t, stats_t)

    def vcf_samples_csr(self, offsets, entries, samples, ref_base, results, n_samples, text=None, text_cap=None):
        """bvc_vcf_samples_csr on host arrays: the sample columns of the called sites' VCF lines.  entries (ENTRY_DTYPE) and samples
        (int32) of site s at offsets[s] .. offsets[s + 1].  text: a uint8 array to format into (e.g. a host_alloc view; default: a new one
        of the size needed); text_cap: what to tell the library instead of its size.  Returns (text, text_off [n_sites + 1], text_len
        [n_sites]): site s's columns are text[text_off[s] : text_off[s] + text_len[s]]."""
        o, e, sm = _as(offsets, np.int64), _as(entries, ENTRY_DTYPE), _as(samples, np.int32)
        r, res = _as(ref_base, np.int8), _as(results, SITE_DTYPE)
        n = len(o) - 1
        assert r.shape == (n,) and res.shape == (n,) and len(e) == len(sm)
        if text is None:
            text = np.zeros(max(1, vcf_samples_need(n_samples, o, res)), dtype=np.uint8)
        cap = len(text) if text_cap is None else int(text_cap)
        off, ln = self._call(self._L.bvc_vcf_samples_csr, False,
                             (n, o, e if len(e) else None, sm if len(sm) else None, r, res, int(n_samples), text, cap),
                             [(None, (n + 1,), np.dtype(np.int64)), (None, (n,), np.dtype(np.int64))])
        return text, off, ln

    def vcf_samples_csr_device(self, offsets_t, entries_t, samples_t, ref_t, results_t, n_samples, text_t, text_off_t=None,
                               text_len_t=None, text_cap=None):
        """The same on device tensors (entries_t / results_t: uint8 views of the records; text_t: uint8, 16-byte aligned; text_off_t /
        text_len_t: int64).  The call waits once for the sum of the slots (BvcError when text_t is too small); the formatting is
        asynchronous on the context's stream.  In overlap mode call join() first."""
        import torch
        ns = offsets_t.numel() - 1
        if text_off_t is None:
            text_off_t = torch.empty(ns + 1, dtype=torch.int64, device=offsets_t.device)
        if text_len_t is None:
            text_len_t = torch.empty(max(1, ns), dtype=torch.int64, device=offsets_t.device)
        cap = text_t.numel() if text_cap is None else int(text_cap)
        self._call(self._L.bvc_vcf_samples_csr, True, (ns, offsets_t, entries_t, samples_t, ref_t, results_t, int(n_samples), text_t, cap,
                                                       text_off_t, text_len_t))
        return text_t, text_off_t, text_len_t

    def _pileup_sample(self, fn, n_positions, n_samples, buf, cap):
        """bvc_pileup_sample_text / bvc_pileup_sample_bgzf: (buf, its offsets [T + 1], text_len [T])."""
        off = np.zeros(n_positions + 1, dtype=np.int64)
        ln = np.zeros(max(1, n_positions), dtype=np.int64)
        cap = len(buf) if cap is None else int(cap)
        self._check(fn(self._h, int(n_samples), _np_ptr(buf) if len(buf) else None, cap, _np_ptr(off), _np_ptr(ln)))
        return buf, off, ln[:n_positions]

    def pileup_sample_text(self, n_positions, n_samples, text, text_cap=None):
        """bvc_pileup_sample_text after a tile finished with sample_text=True: the called positions' sample columns into text (uint8 array).
        Returns (text, text_off [T + 1], text_len [T])."""
        return self._pileup_sample(self._L.bvc_pileup_sample_text, n_positions, n_samples, text, text_cap)

    def bgzf_deflate(self, data, piece_off, piece_len, comp=None, comp_cap=None):
        """bvc_bgzf_deflate on host arrays: piece i = data[piece_off[i] : piece_off[i] + piece_len[i]] (uint8) as BGZF blocks.  comp: a uint8
        array to write into (default: a new one of the bound); comp_cap: what to tell the library instead of its size.  Returns (comp,
        comp_off [n + 1]): piece i's blocks are comp[comp_off[i] : comp_off[i + 1]]."""
        d, o, ln = _as(data, np.uint8), _as(piece_off, np.int64), _as(piece_len, np.int64)
        n = len(o)
        assert ln.shape == (n,)
        if comp is None:
            comp = np.zeros(max(1, sum(bgzf_bound(x) for x in ln)), dtype=np.uint8)
        cap = len(comp) if comp_cap is None else int(comp_cap)
        off, = self._call(self._L.bvc_bgzf_deflate, False, (n, d if len(d) else None, o if n else None, ln if n else None, comp, cap),
                          [(None, (n + 1,), np.dtype(np.int64))])
        return comp, off

    def bgzf_deflate_device(self, data_t, piece_off_t, piece_len_t, comp_t, comp_off_t=None, comp_cap=None):
        """The same on device tensors (data_t / comp_t: uint8, any alignment; piece_off_t / piece_len_t / comp_off_t: int64).  The call
        waits for the pieces' lengths (BvcError when comp_t is smaller than the sum of their bounds) and for its small block table to
        have gone up; the blocks and comp_off are written asynchronously on the context's stream."""
        import torch
        n = piece_off_t.numel()
        if comp_off_t is None:
            comp_off_t = torch.empty(n + 1, dtype=torch.int64, device=comp_t.device)
        cap = comp_t.numel() if comp_cap is None else int(comp_cap)
        self._call(self._L.bvc_bgzf_deflate, True, (n, data_t, piece_off_t, piece_len_t, comp_t, cap, comp_off_t))
        return comp_t, comp_off_t

    def pileup_sample_bgzf(self, n_positions, n_samples, comp, comp_cap=None):
        """bvc_pileup_sample_bgzf after a tile finished with sample_text=True: the called positions' sample columns as BGZF blocks into comp
        (uint8 array).  Returns (comp, comp_off [T + 1], text_len [T])."""
        return self._pileup_sample(self._L.bvc_pileup_sample_bgzf, n_positions, n_samples, comp, comp_cap)

    def bgzf_code_lengths(self, counts, limit):
        """bvc_bgzf_code_lengths (include/bvc_bgzf_codes.h): the code lengths (uint8, the shape of counts) the device deflate encoder's rule gives each row of counts
        (uint32 [n_sets, n_symbols] or one row), none above limit (docs/BGZF_DYNAMIC.md)."""
        c = _as(counts, np.uint32)
        rows = c.reshape(-1, c.shape[-1]) if c.ndim else c.reshape(1, 1)
        out = np.zeros(rows.shape, dtype=np.uint8)
        self._check(self._L.bvc_bgzf_code_lengths(self._h, rows.shape[0], _np_ptr(rows) if rows.size else None, rows.shape[1], int(limit),
                                                  _np_ptr(out) if out.size else None))
        return out.reshape(c.shape)

    # ---- packed tiles: one byte per sample (base << 6 | qual, qual <= 62; 0xFF = no observation) ----
    def pack_dense_device(self, bases_t, quals_t, packed_t=None):
        """Two-byte device tile -> packed device tile.  Returns (packed_t, n_unrepresentable)."""
        import torch
        ns, n, stride_in = _tile(bases_t, quals_t)
        if packed_t is None:
            stride = (n + 127) // 128 * 128
            packed_t = torch.empty((ns, stride), dtype=torch.uint8, device=bases_t.device)[:, :n]
        bad = C.c_int64(0)
        self._call(self._L.bvc_pack_dense, True, (ns, n, stride_in, bases_t, quals_t, packed_t.stride(0), packed_t, C.byref(bad)))
        return packed_t, int(bad.value)

    def _lrt_dense_packed(self, device, ns, n, stride, p, r, min_af, res=None):
        return self._call(self._L.bvc_lrt_dense_packed, device, (ns, n, stride, p, r, float(min_af)), [(res, (ns,), SITE_DTYPE)])[0]

    def lrt_dense_packed(self, packed, ref_base, min_af):
        """Host (numpy) packed tile [n_sites, n_samples] uint8."""
        p = _as(packed, np.uint8)
        ns, n = p.shape
        return self._lrt_dense_packed(False, ns, n, n, p, _as(ref_base, np.int8), min_af)

    def lrt_dense_packed_device(self, packed_t, ref_t, min_af, results_t=None):
        return self._lrt_dense_packed(True, *_tile(packed_t), packed_t, ref_t, min_af, results_t)

    def _lrt_dense_groups_packed(self, device, ns, n, stride, p, r, min_af, g, n_groups, res=None, gres=None):
        return tuple(self._call(self._L.bvc_lrt_dense_groups_packed, device, (ns, n, stride, p, r, float(min_af), g, int(n_groups)),
                                [(res, (ns,), SITE_DTYPE), (gres, (ns, n_groups), GROUP_DTYPE)]))

    def lrt_dense_groups_packed(self, packed, ref_base, min_af, group_of_sample, n_groups):
        p = _as(packed, np.uint8)
        return self._lrt_dense_groups_packed(False, p.shape[0], p.shape[1], p.shape[1], p, _as(ref_base, np.int8), min_af,
                                             _as(group_of_sample, np.uint8), n_groups)

    def lrt_dense_groups_packed_device(self, packed_t, ref_t, min_af, group_t, n_groups, results_t=None, grp_results_t=None):
        return self._lrt_dense_groups_packed(True, *_tile(packed_t), packed_t, ref_t, min_af, group_t, n_groups, results_t,
                                             grp_results_t)

    # ---- the two stages on their own
    def hist_dense(self, bases, quals):
        b, q = _as(bases, np.int8), _as(quals, np.int8)
        out = np.zeros((b.shape[0], NCLASS), dtype=np.uint32)
        self._call(self._L.bvc_hist_dense, False, (b.shape[0], b.shape[1], b.shape[1], b, q, out))
        return out

    def hist_dense_device(self, bases_t, quals_t, counts_t=None):
        import torch
        ns, n = bases_t.shape
        if counts_t is None:
            counts_t = torch.empty((ns, NCLASS), dtype=torch.int32, device=bases_t.device)
        self._call(self._L.bvc_hist_dense, True, (ns, n, bases_t.stride(0), bases_t, quals_t, counts_t))
        return counts_t

    def hist_dense_packed_device(self, packed_t, counts_t=None):
        import torch
        ns, n = packed_t.shape
        if counts_t is None:
            counts_t = torch.empty((ns, NCLASS), dtype=torch.int32, device=packed_t.device)
        self._call(self._L.bvc_hist_dense_packed, True, (ns, n, packed_t.stride(0), packed_t, counts_t))
        return counts_t

    def _lrt_hist(self, device, ns, c, r, min_af, cb=None, nc=None, res=None):
        return self._call(self._L.bvc_lrt_hist, device, (ns, c, r, float(min_af), cb, nc), [(res, (ns,), SITE_DTYPE)])[0]

    def lrt_hist(self, counts, ref_base, min_af, base_comb=None, n_comb=None):
        c = _as(counts, np.uint32).reshape(-1, NCLASS)
        cb = nc = None
        if base_comb is not None:
            cb = _as(base_comb, np.int8).reshape(-1, 4)
            nc = _as(n_comb, np.uint8)
        return self._lrt_hist(False, c.shape[0], c, _as(ref_base, np.int8), min_af, cb, nc)

    def lrt_hist_device(self, counts_t, ref_t, min_af, results_t=None):
        """Stage 2 alone on device tensors: counts_t int32/uint32 [n_sites, 512]; asynchronous on the stream."""
        return self._lrt_hist(True, counts_t.shape[0], counts_t, ref_t, min_af, res=results_t)

    # ---- the producer: temp batches parsed on the device (host pointers only)
    def pileup_tile(self, text, line_start, sample0, n_in_batch, ref_base, min_af, carry_in=(0, 0, 0, 0, 0), group_of_sample=None,
                    n_groups=0, called_only=False, stats=False, sample_text=False):
        """bvc_pileup_begin + bvc_pileup_finish on one tile of temp-batch pileup text (include/bvc.h).  text: bytes;
        line_start: uint32 [n_batches, n_positions + 1].  Returns None when a line is not regular (BVC_PILEUP_IRREGULAR), else a
        dict: entry_off, tally [T, 32], entries (structured), samples, indels (sorted by entry), results, grp_results, carry_out.
        stats=True (needs called_only=True): bvc_pileup_finish_called_stats -- key "stats", STATS_DTYPE [T].
        sample_text=True: bvc_pileup_finish_called_text -- "stats" too, no entries / samples; pileup_sample_text() then formats the columns."""
        ls = _as(line_start, np.uint32)
        rc, T, ne, ni = self._pileup_begin(self._L.bvc_pileup_begin, text, ls, _as(sample0, np.int32), _as(n_in_batch, np.int32))
        if rc == 1:
            return None
        self._check(rc)
        return self._pileup_finish(T, ne, ni, 0, ref_base, min_af, carry_in, group_of_sample, n_groups, called_only, stats=stats, sample_text=sample_text)

    def pileup_tile_bin(self, records, rec_start, sample0, n_in_batch, ref_base, min_af, carry_in=(0, 0, 0, 0, 0), group_of_sample=None,
                        n_groups=0, called_only=False, stats=False, sample_text=False):
        """bvc_pileup_begin_bin + bvc_pileup_finish on one tile of binary temp-batch records (include/bvc.h).  records: bytes;
        rec_start: uint32 [n_batches, n_positions + 1].  Returns the dict of pileup_tile (indels' text_off are offsets into records);
        raises BvcError (status BVC_ERR_DATA = -5: a malformed record, BVC_ERR_ARG = -1: a rec_start that does not fit)."""
        rs = _as(rec_start, np.uint32)
        if rs.ndim != 2 or rs.shape[1] < 1:
            raise ValueError("rec_start must be [n_batches, n_positions + 1]")
        s0, nib = _as(sample0, np.int32), _as(n_in_batch, np.int32)
        if s0.shape != (rs.shape[0],) or nib.shape != (rs.shape[0],):
            raise ValueError("sample0 / n_in_batch must be [n_batches]")
        rc, T, ne, ni = self._pileup_begin(self._L.bvc_pileup_begin_bin, records, rs, s0, nib)
        self._check(rc)
        return self._pileup_finish(T, ne, ni, 0, ref_base, min_af, carry_in, group_of_sample, n_groups, called_only, stats=stats, sample_text=sample_text)

    def _pileup_begin(self, fn, data, start, s0, nib):
        """bvc_pileup_begin (text, line_start) / bvc_pileup_begin_bin (records, rec_start): (rc, n_positions, n_entries, n_indels)."""
        nb, T = start.shape[0], start.shape[1] - 1
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        ne, ni = C.c_int64(0), C.c_int64(0)
        rc = fn(self._h, *_pointers((buf if len(buf) else None, len(buf), start, s0, nib, nb, T, C.byref(ne), C.byref(ni)), _np_ptr))
        return rc, T, ne.value, ni.value

    def _pileup_finish(self, T, n_entries, n_indels, indel_text_bytes, ref_base, min_af, carry_in, group_of_sample, n_groups,
                       called_only=False, called_cap=None, stats=False, sample_text=False):
        """called_only: bvc_pileup_finish_called -- `entries` / `samples` hold the called positions' entries only, position t's at
        called_off[t] .. called_off[t + 1] (key "called_off").  stats (with called_only): bvc_pileup_finish_called_stats, key "stats".
        sample_text (alone): bvc_pileup_finish_called_text -- key "stats", and "entries" / "samples" stay empty: the columns stay on the device."""
        if sample_text and (called_only or stats):
            raise ValueError("sample_text=True stands alone (bvc_pileup_finish_called_text delivers the statistics itself)")
        if stats and not called_only:
            raise ValueError("stats=True needs called_only=True (bvc_pileup_finish_called_stats)")
        r = _as(ref_base, np.int8)
        assert r.shape == (T,)
        entry_off = np.zeros(T + 1, dtype=np.int64)
        tally = np.zeros((T, 32), dtype=np.int32)
        entries = np.zeros(max(1, n_entries), dtype=ENTRY_DTYPE)
        samples = np.zeros(max(1, n_entries), dtype=np.int32)
        indels = np.zeros(max(1, n_indels), dtype=INDEL_DTYPE)
        itext = np.zeros(max(1, indel_text_bytes), dtype=np.uint8)
        res = np.zeros(T, dtype=SITE_DTYPE)
        gres = np.zeros((T, max(1, n_groups)), dtype=GROUP_DTYPE)
        g = _as(group_of_sample, np.uint8) if n_groups else np.zeros(0, dtype=np.uint8)
        cin = np.asarray(carry_in, dtype=np.uint8)
        cout = np.zeros(5, dtype=np.uint8)
        fn = self._L.bvc_pileup_finish
        args = [r, float(min_af), cin, cout, g if n_groups else None, len(g), int(n_groups), entry_off, tally]
        if called_only:
            fn = self._L.bvc_pileup_finish_called_stats if stats else self._L.bvc_pileup_finish_called
            called_off = np.zeros(T + 1, dtype=np.int64)
            args += [called_off, n_entries if called_cap is None else int(called_cap)]
        if sample_text:
            fn = self._L.bvc_pileup_finish_called_text
            stats = True
        else:
            args += [entries, samples]
        args += [indels, itext if indel_text_bytes else None, res, gres if n_groups else None]
        if stats:
            st = np.zeros(max(1, T), dtype=STATS_DTYPE)
            args.append(st)
        self._check(fn(self._h, *_pointers(args, _np_ptr)))
        n_kept = int(called_off[T]) if called_only else (0 if sample_text else n_entries)
        ind = indels[:n_indels]
        ind = ind[np.argsort(ind["entry"], kind="stable")]
        out = dict(entry_off=entry_off, tally=tally, entries=entries[:n_kept], samples=samples[:n_kept], indels=ind, results=res,
                   grp_results=gres if n_groups else None, carry_out=[int(x) for x in cout], indel_text=itext[:indel_text_bytes].tobytes())
        if called_only:
            out["called_off"] = called_off
        if stats:
            out["stats"] = st[:T]
        return out

    def pileup_begin_bgzf(self, comp, blocks, blocks_of_batch, skip_bytes, sample0, n_in_batch, max_positions, reset):
        """bvc_pileup_begin_bgzf.  comp: bytes; blocks: [(comp_off, comp_len, isize)] batch after batch.  Returns a dict with rc
        (0, 1 = irregular, negative = error), T, lines (per batch) and the sizes bvc_pileup_finish needs."""
        tab, _ = _block_table(blocks, consecutive=False)
        if isinstance(comp, np.ndarray):                         # e.g. a view of page-locked memory (host_alloc): used where it lies
            buf = comp
            comp_len = len(buf)
        else:
            buf = np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8)
            comp_len = len(buf) - 8
        bob = _as(blocks_of_batch, np.int32)
        nb = len(bob)
        sk = _as(skip_bytes, np.int32) if skip_bytes is not None else None
        lines = np.zeros(max(1, nb), dtype=np.int32)
        T, ne, ni, nt = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = self._L.bvc_pileup_begin_bgzf(self._h, *_pointers(
            (buf, comp_len, tab, bob, sk, _as(sample0, np.int32), _as(n_in_batch, np.int32), nb, int(max_positions), int(bool(reset)),
             C.byref(T), lines, C.byref(ne), C.byref(ni), C.byref(nt)), _np_ptr))
        return dict(rc=rc, T=T.value, lines=lines[:nb].copy(), n_entries=ne.value, n_indels=ni.value, indel_text_bytes=nt.value,
                    error=self._L.bvc_last_error(self._h).decode() if rc < 0 else "")

    def pileup_text(self, n_batches, T):
        need = C.c_int64(0)
        self._check(self._L.bvc_pileup_text(self._h, None, 0, C.byref(need), None))
        text = np.zeros(max(1, need.value), dtype=np.uint8)
        ls = np.zeros((n_batches, T + 1), dtype=np.uint32)
        self._check(self._L.bvc_pileup_text(self._h, _np_ptr(text), need.value, C.byref(need), _np_ptr(ls)))
        return text[:need.value].tobytes(), ls

    def inflate_blocks(self, comp, blocks):
        """Raw-deflate streams inflated on the device.  comp: bytes; blocks: [(comp_off, comp_len, isize)] -- outputs are laid out one
        after the other.  Returns (list of bytes, status array)."""
        tab, at = _block_table(blocks, consecutive=True)
        buf = np.frombuffer(bytes(comp) + b"\0" * 8, dtype=np.uint8)
        out = np.zeros(max(1, at), dtype=np.uint8)
        status = np.zeros(max(1, len(blocks)), dtype=np.uint32)
        self._call(self._L.bvc_inflate_blocks, False, (buf, len(buf), tab, len(blocks), out, at, status))
        return [out[int(t["out_off"]):int(t["out_off"]) + int(t["isize"])].tobytes() for t in tab[:len(blocks)]], status[:len(blocks)]

    def bam_pileup(self, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq, records=None, records_cap=None,
                   rec_start=None, sample_status=None):
        """bvc_bam_pileup (include/bvc_bam.h): the inflated BAM records of a batch of samples -> the batch's binary temp-batch records.
        numpy arrays (synchronous) or tensors on this context's device (asynchronous but for one wait): bam uint8, sample_off and
        sample_end int64 [n], sample_eof uint8 [n], rid int32 [n], positions int32 (1-based, ascending), refseq uint8 (the reference's characters).
        records / rec_start / sample_status: buffers to write into (uint8, uint32 [P + 1], uint32 [n]); without records the call is made
        twice, the second time with a buffer of the size the first reports.  records_cap: what to tell the library instead of len(records).
        Returns (rc, records, rec_start, sample_status, records_needed): rc 0, or BAM_MORE (2) when a sample's status is 2 or records is
        too small -- nothing is written then.  Raises BvcError for the errors (status BVC_ERR_DATA = -5: a sample of status 3 or 4)."""
        return self._bam_pileup(self._L.bvc_bam_pileup, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq, records,
                                records_cap, rec_start, sample_status)

    def _bam_pileup(self, fn, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq, records, records_cap, rec_start,
                    sample_status):
        """bam_pileup and bam_pileup_text: fn is bvc_bam_pileup or its twin of the same arguments."""
        device = hasattr(bam, "data_ptr")
        if device:
            import torch
            new = lambda n, dt: torch.zeros(max(1, n), dtype=dt, device=bam.device)
            u8, u32, size = torch.uint8, torch.int32, lambda a: a.numel()
        else:
            bam, sample_off, sample_end = _as(bam, np.uint8), _as(sample_off, np.int64), _as(sample_end, np.int64)
            sample_eof, rid = _as(sample_eof, np.uint8), _as(rid, np.int32)
            positions, refseq = _as(positions, np.int32), _as(refseq, np.uint8)
            new = lambda n, dt: np.zeros(max(1, n), dtype=dt)
            u8, u32, size = np.uint8, np.uint32, len
        n, P = size(rid), size(positions)
        if size(sample_off) != n or size(sample_end) != n or size(sample_eof) != n:
            raise ValueError("sample_off, sample_end and sample_eof must be [n_samples]")
        rec_start = new(P + 1, u32) if rec_start is None else rec_start
        sample_status = new(n, u32) if sample_status is None else sample_status
        need = C.c_int64(0)
        ptr = _dev_ptr if device else _np_ptr
        opt = lambda a: a if a is not None and size(a) else None

        def call(buf, cap):
            rc = fn(self._h, n, *_pointers((opt(bam), size(bam), opt(sample_off), opt(sample_end), opt(sample_eof), opt(rid), int(beg0), int(end0),
                                                               int(min_mapq), P, opt(positions), int(rg_s), opt(refseq), size(refseq), opt(buf), cap),
                                                              ptr), C.byref(need), ptr(rec_start), ptr(sample_status) if n else None,
                                        BVC_PTR_DEVICE if device else BVC_PTR_HOST)
            if rc not in (0, BAM_MORE):
                self._check(rc)
            return rc
        if records is None:
            rc = call(None, 0)
            if rc == 0 or need.value == 0:
                return rc, new(0, u8)[:0], rec_start, sample_status, need.value
            records = new(need.value, u8)
        rc = call(records, size(records) if records_cap is None else int(records_cap))
        return rc, records[:need.value] if rc == 0 else records, rec_start, sample_status, need.value

    def bam_pileup_text(self, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq, text=None, text_cap=None,
                        line_start=None, sample_status=None):
        """bvc_bam_pileup_text (include/bvc_bam_text.h): the same records -> the batch's lines in the text temp-batch form.  Everything as
        bam_pileup, with text / text_cap / line_start in the places of records / records_cap / rec_start.  Returns (rc, text, line_start,
        sample_status, text_needed)."""
        return self._bam_pileup(self._L.bvc_bam_pileup_text, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq,
                                text, text_cap, line_start, sample_status)

    def bam_pileup_text_bgzf(self, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq,
                             text=None, text_cap=None, line_start=None, sample_status=None):
        """bvc_bam_pileup_text_bgzf: the same from BGZF blocks still compressed.  comp: uint8 array; blocks: a BLOCK_DTYPE table (out_off:
        where each block's output lies among the bam_bytes inflated bytes).  Host arrays only.  Without text the call is made twice, as
        bam_pileup makes it.  Returns (rc, text, line_start, sample_status, text_needed)."""
        return self._bam_pileup_bgzf(self._L.bvc_bam_pileup_text_bgzf, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq,
                                     positions, rg_s, refseq, text, text_cap, line_start, sample_status)

    def bam_pileup_bgzf(self, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq,
                        records=None, records_cap=None, rec_start=None, sample_status=None):
        """bvc_bam_pileup_bgzf (include/bvc_bam.h): bam_pileup_text_bgzf's binary twin.  Returns (rc, records, rec_start, sample_status,
        records_needed)."""
        return self._bam_pileup_bgzf(self._L.bvc_bam_pileup_bgzf, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq,
                                     positions, rg_s, refseq, records, records_cap, rec_start, sample_status)

    @staticmethod
    def _bgzf_inputs(comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq):
        """The arguments the _bgzf calls share, from comp to refseq_len, as host arrays and numbers in the header's order."""
        comp, tab = _as(comp, np.uint8), np.ascontiguousarray(blocks, dtype=BLOCK_DTYPE)
        sample_off, sample_end, sample_eof, rid = _as(sample_off, np.int64), _as(sample_end, np.int64), _as(sample_eof, np.uint8), _as(rid, np.int32)
        positions, refseq = _as(positions, np.int32), _as(refseq, np.uint8)
        n, P = len(rid), len(positions)
        if len(sample_off) != n or len(sample_end) != n or len(sample_eof) != n:
            raise ValueError("sample_off, sample_end and sample_eof must be [n_samples]")
        opt = lambda a: a if a is not None and len(a) else None
        return n, P, (opt(comp), len(comp), opt(tab), len(tab), int(bam_bytes), opt(sample_off), opt(sample_end), opt(sample_eof), opt(rid), int(beg0),
                      int(end0), int(min_mapq), P, opt(positions), int(rg_s), opt(refseq), len(refseq))

    def _bam_pileup_bgzf(self, fn, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq,
                         text, text_cap, line_start, sample_status):
        n, P, shared = self._bgzf_inputs(comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq)
        line_start = np.zeros(P + 1, dtype=np.uint32) if line_start is None else line_start
        sample_status = np.zeros(max(1, n), dtype=np.uint32) if sample_status is None else sample_status
        need = C.c_int64(0)

        def call(buf, cap):
            rc = fn(self._h, n, *_pointers((*shared, buf if buf is not None and len(buf) else None, cap), _np_ptr), C.byref(need),
                    _np_ptr(line_start), _np_ptr(sample_status) if n else None)
            if rc not in (0, BAM_MORE):
                self._check(rc)
            return rc
        if text is None:
            rc = call(None, 0)
            if rc == 0 or need.value == 0:
                return rc, np.zeros(0, dtype=np.uint8), line_start, sample_status, need.value
            text = np.zeros(need.value, dtype=np.uint8)
        rc = call(text, len(text) if text_cap is None else int(text_cap))
        return rc, text[:need.value] if rc == 0 else text, line_start, sample_status, need.value

    def bam_pileup_bgzf_deflate(self, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq,
                                piece_pos, text=False, out=None, out_cap=None, out_off=None, piece_bytes=None, sample_status=None):
        """bvc_bam_pileup_bgzf_deflate / bvc_bam_pileup_text_bgzf_deflate (text=True; include/bvc_bam_deflate.h): bam_pileup_bgzf /
        bam_pileup_text_bgzf with the batch deflated on the device into finished BGZF blocks.  piece_pos: int32 [n_pieces + 1], indices
        into positions from 0 to len(positions); piece i's blocks are out[out_off[i]:out_off[i + 1]].  out / out_off / piece_bytes /
        sample_status: buffers to write into (uint8, int64 [n_pieces + 1], int64 [n_pieces], uint32 [n]); without out the call is made
        with out_cap 0 and the blocks it leaves in the context are fetched (bam_pileup_deflate_fetch).  out_cap: what to tell the
        library instead of len(out).  Returns (rc, out, out_off, piece_bytes, sample_status, out_needed): rc 0, or BAM_MORE (2) when a
        sample's status is 2 (out_needed 0) or out is too small (out_needed the packed size; out_off and piece_bytes are written).
        Raises BvcError for the errors."""
        n, _, shared = self._bgzf_inputs(comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq)
        piece_pos = _as(piece_pos, np.int32)
        if len(piece_pos) < 1:
            raise ValueError("piece_pos must be [n_pieces + 1]")
        k = len(piece_pos) - 1
        out_off = np.zeros(k + 1, dtype=np.int64) if out_off is None else out_off
        piece_bytes = np.zeros(max(1, k), dtype=np.int64) if piece_bytes is None else piece_bytes
        sample_status = np.zeros(max(1, n), dtype=np.uint32) if sample_status is None else sample_status
        need = C.c_int64(0)
        fn = self._L.bvc_bam_pileup_text_bgzf_deflate if text else self._L.bvc_bam_pileup_bgzf_deflate
        cap = (len(out) if out is not None else 0) if out_cap is None else int(out_cap)
        rc = fn(self._h, n, *_pointers((*shared, k, piece_pos, out if out is not None and len(out) else None, cap), _np_ptr), C.byref(need),
                _np_ptr(out_off), _np_ptr(piece_bytes), _np_ptr(sample_status) if n else None)
        if rc not in (0, BAM_MORE):
            self._check(rc)
        if out is None:
            out = np.zeros(0, dtype=np.uint8)
            if rc == BAM_MORE and need.value > 0 and out_cap is None:
                out = self.bam_pileup_deflate_fetch(need.value)
                rc = 0
        return rc, out[:need.value] if rc == 0 else out, out_off, piece_bytes, sample_status, need.value

    def bam_pileup_deflate_fetch(self, size, out=None, out_cap=None):
        """bvc_bam_pileup_deflate_fetch: the blocks the last bam_pileup_bgzf_deflate left in the context when out was too small, `size`
        bytes (its out_needed), as a uint8 array.  Raises BvcError (BVC_ERR_ARG) when nothing is kept or the room is too small."""
        out = np.zeros(int(size), dtype=np.uint8) if out is None else out
        self._check(self._L.bvc_bam_pileup_deflate_fetch(self._h, _np_ptr(out) if len(out) else None, len(out) if out_cap is None else int(out_cap)))
        return out

    def bam_pileup_bgzf_store(self, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq,
                              store, batch, sample_status=None):
        """bvc_bam_pileup_bgzf_store (include/bvc_store.h): bam_pileup_bgzf, but the records and rec_start stay on the device as batch `batch`
        of `store` (a Store).  Returns (rc, sample_status, records_bytes): rc 0, or BAM_MORE (2) -- nothing is put then.  Raises BvcError for
        the errors."""
        n, _, shared = self._bgzf_inputs(comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq)
        sample_status = np.zeros(max(1, n), dtype=np.uint32) if sample_status is None else sample_status
        need = C.c_int64(0)
        rc = self._L.bvc_bam_pileup_bgzf_store(self._h, n, *_pointers(shared, _np_ptr), store._h, int(batch), C.byref(need),
                                               _np_ptr(sample_status) if n else None)
        if rc not in (0, BAM_MORE):
            self._check(rc)
        return rc, sample_status, need.value

    def pileup_begin_store(self, store, t0, n_positions):
        """bvc_pileup_begin_store (include/bvc_store.h): positions [t0, t0 + n_positions) of every batch of the sealed Store gathered into
        this context's tile.  Returns (n_entries, n_indels, indel_text_bytes): what pileup_finish_store needs."""
        ne, ni, nt = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self._L.bvc_pileup_begin_store(self._h, store._h, int(t0), int(n_positions), C.byref(ne), C.byref(ni), C.byref(nt)))
        return ne.value, ni.value, nt.value

    def pileup_tile_store(self, store, t0, n_positions, ref_base, min_af, carry_in=(0, 0, 0, 0, 0), group_of_sample=None, n_groups=0,
                          called_only=False, stats=False, sample_text=False):
        """pileup_begin_store + one of the finish calls: the dict of pileup_tile_bin, the indel records' text_off offsets into its
        "indel_text" (the tile's records are on the device only)."""
        ne, ni, nt = self.pileup_begin_store(store, t0, n_positions)
        return self._pileup_finish(int(n_positions), ne, ni, nt, ref_base, min_af, carry_in, group_of_sample, n_groups, called_only, stats=stats,
                                   sample_text=sample_text)

    def bam_popmatrix(self, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, ref, alt, rg_s, refseq_len, matrix=None,
                      row_stride=None, sample_status=None):
        """bvc_bam_popmatrix (include/bvc_popmatrix.h): the inflated BAM records of a batch of samples and a position file's lines -> one
        row of '0' / '1' / '.' per sample.  numpy arrays (synchronous) or tensors on this context's device (asynchronous but for one wait
        at the end): the sample arrays as bam_pileup takes them; positions int32 (1-based, not descending, repeats allowed), ref / alt
        uint8 [P] (the lines' REF and ALT characters).  matrix / sample_status: buffers to write into (uint8 of at least n * row_stride
        bytes, uint32 [n]); row_stride defaults to P.  Returns (rc, matrix, sample_status): rc 0, or BAM_MORE (2) when a sample's status
        is 2; the rows of samples with status 0 or 1 are defined either way.  Raises BvcError for the errors (status BVC_ERR_DATA = -5: a
        sample of status 3 or 4; the buffers given keep what the call wrote)."""
        device = hasattr(bam, "data_ptr")
        if device:
            import torch
            new = lambda n, dt: torch.zeros(max(1, n), dtype=dt, device=bam.device)
            u8, u32, size = torch.uint8, torch.int32, lambda a: a.numel()
        else:
            bam, sample_off, sample_end = _as(bam, np.uint8), _as(sample_off, np.int64), _as(sample_end, np.int64)
            sample_eof, rid = _as(sample_eof, np.uint8), _as(rid, np.int32)
            positions, ref, alt = _as(positions, np.int32), _as(ref, np.uint8), _as(alt, np.uint8)
            new = lambda n, dt: np.zeros(max(1, n), dtype=dt)
            u8, u32, size = np.uint8, np.uint32, len
        n, P = size(rid), size(positions)
        if size(sample_off) != n or size(sample_end) != n or size(sample_eof) != n:
            raise ValueError("sample_off, sample_end and sample_eof must be [n_samples]")
        if size(ref) != P or size(alt) != P:
            raise ValueError("ref and alt must be [n_positions]")
        row_stride = P if row_stride is None else int(row_stride)
        matrix = new(n * max(row_stride, 0), u8) if matrix is None else matrix
        sample_status = new(n, u32) if sample_status is None else sample_status
        ptr = _dev_ptr if device else _np_ptr
        opt = lambda a: a if a is not None and size(a) else None
        rc = self._L.bvc_bam_popmatrix(self._h, n, *_pointers((opt(bam), size(bam), opt(sample_off), opt(sample_end), opt(sample_eof), opt(rid), int(beg0),
                                                              int(end0), int(min_mapq), P, opt(positions), opt(ref), opt(alt), int(rg_s), int(refseq_len),
                                                              matrix, row_stride, sample_status if n else None), ptr),
                                       BVC_PTR_DEVICE if device else BVC_PTR_HOST)
        if rc not in (0, BAM_MORE):
            self._check(rc)
        return rc, matrix, sample_status

    def bam_popmatrix_bgzf(self, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, ref, alt, rg_s,
                           refseq_len):
        """bvc_bam_popmatrix_bgzf: the same from BGZF blocks still compressed.  comp: uint8 array; blocks: a BLOCK_DTYPE table (out_off: where
        each block's output lies among the bam_bytes inflated bytes).  Host arrays only.  Returns (rc, matrix [n, P], sample_status)."""
        comp, tab = _as(comp, np.uint8), np.ascontiguousarray(blocks, dtype=BLOCK_DTYPE)
        sample_off, sample_end, sample_eof, rid = _as(sample_off, np.int64), _as(sample_end, np.int64), _as(sample_eof, np.uint8), _as(rid, np.int32)
        positions, ref, alt = _as(positions, np.int32), _as(ref, np.uint8), _as(alt, np.uint8)
        n, P = len(rid), len(positions)
        matrix, status = np.zeros((max(1, n), max(1, P)), dtype=np.uint8), np.zeros(max(1, n), dtype=np.uint32)
        opt = lambda a: a if len(a) else None
        rc = self._L.bvc_bam_popmatrix_bgzf(self._h, n, *_pointers((opt(comp), len(comp), opt(tab), len(tab), int(bam_bytes), opt(sample_off), opt(sample_end),
                                                                   opt(sample_eof), opt(rid), int(beg0), int(end0), int(min_mapq), P, opt(positions), opt(ref),
                                                                   opt(alt), int(rg_s), int(refseq_len), matrix, max(1, P) if n and P else P, status), _np_ptr))
        if rc not in (0, BAM_MORE):
            self._check(rc)
        return rc, matrix[:n, :P], status[:n]

    def bam_counts(self, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq_len, counts, tally,
                   group_of_sample=None, n_groups=0, sample_status=None, group_depth=None, n_quals=None):
        """bvc_bam_counts (include/bvc_bam_counts.h): the inflated BAM records of a batch of samples ADDED into counts ([P, 512], or
        [P, n_groups + 1, 512] with groups; 4-byte integers) and tally (TALLY_DTYPE [P], or 12 words a position), in place.  numpy arrays
        (synchronous) or tensors on this context's device (the adds are enqueued when it returns); the sample arrays and positions as
        bam_pileup takes them, group_of_sample uint8 [n].  Returns (rc, sample_status): rc 0, or BAM_MORE (2) when a sample's status is 2
        -- nothing is added then.  Raises BvcError for the errors (status BVC_ERR_DATA = -5: a sample of status 3 or 4; nothing is added).
        group_depth: bam_counts_depth's third array -- the call is then bvc_bam_counts_depth.  n_quals: the call is bvc_bam_counts_quals
        (bam_counts_quals below), whose group_depth may be None without groups."""
        device = hasattr(bam, "data_ptr")
        outs = (counts, tally) if group_depth is None else (counts, tally, group_depth)
        if device:
            import torch
            new = lambda n, dt: torch.zeros(max(1, n), dtype=dt, device=bam.device)
            u32, size = torch.int32, lambda a: a.numel()
        else:
            bam, sample_off, sample_end = _as(bam, np.uint8), _as(sample_off, np.int64), _as(sample_end, np.int64)
            sample_eof, rid, positions = _as(sample_eof, np.uint8), _as(rid, np.int32), _as(positions, np.int32)
            group_of_sample = None if group_of_sample is None else _as(group_of_sample, np.uint8)
            new = lambda n, dt: np.zeros(max(1, n), dtype=dt)
            u32, size = np.uint32, len
            if not all(isinstance(a, np.ndarray) and a.flags.c_contiguous for a in outs):
                raise ValueError("counts and tally" + (" and group_depth" if group_depth is not None else "") +
                                 " must be contiguous arrays (they are added to in place)")
        n, P = size(rid), size(positions)
        if size(sample_off) != n or size(sample_end) != n or size(sample_eof) != n or (group_of_sample is not None and size(group_of_sample) != n):
            raise ValueError("sample_off, sample_end, sample_eof and group_of_sample must be [n_samples]")
        sample_status = new(n, u32) if sample_status is None else sample_status
        ptr = _dev_ptr if device else _np_ptr
        opt = lambda a: a if a is not None and size(a) else None
        fn = self._L.bvc_bam_counts if group_depth is None else self._L.bvc_bam_counts_depth
        quals = ()
        if n_quals is not None:
            fn, quals, outs = self._L.bvc_bam_counts_quals, (int(n_quals),), (counts, tally, group_depth)
        rc = fn(self._h, n, *_pointers((opt(bam), size(bam), opt(sample_off), opt(sample_end), opt(sample_eof), opt(rid), int(beg0), int(end0), int(min_mapq), P,
                                        opt(positions), int(rg_s), int(refseq_len), opt(group_of_sample), int(n_groups), *quals, *outs,
                                        sample_status if n else None), ptr),
                BVC_PTR_DEVICE if device else BVC_PTR_HOST)
        if rc not in (0, BAM_MORE):
            self._check(rc)
        return rc, sample_status

    def bam_counts_depth(self, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq_len, counts, tally,
                         group_depth, group_of_sample, n_groups, sample_status=None):
        """bvc_bam_counts_depth (include/bvc_bam_group_depth.h): bam_counts into ONE slot of counts ([P, 512]) and tally, and the covered
        observations of each group per base ADDED into group_depth ([P, n_groups, 4]; 4-byte integers), in place.  n_groups 1..32; a label
        >= n_groups adds no depth.  Arrays, return value and errors as bam_counts."""
        if group_depth is None:
            raise ValueError("group_depth must be an array (bam_counts is the call without one)")
        return self.bam_counts(bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq_len, counts, tally,
                               group_of_sample, n_groups, sample_status, group_depth)

    def bam_counts_quals(self, bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq_len, n_quals, counts, tally,
                         group_depth=None, group_of_sample=None, n_groups=0, sample_status=None):
        """bvc_bam_counts_quals (include/bvc_site_acc_quals.h): bam_counts into NARROW rows of counts ([P, 4, n_quals]; n_quals a multiple
        of 4 in 4..128) and tally, and with n_groups 1..32 the groups' depths into group_depth ([P, n_groups, 4]), in place.  A batch with a
        counted observation of quality n_quals..127 is refused (BvcError of status BVC_ERR_DATA = -5, that sample's status 5) and adds
        nothing.  Arrays, return value and the other errors as bam_counts."""
        if (group_depth is None) != (not n_groups):
            raise ValueError("group_depth goes with n_groups 1..32")
        outs = (counts, tally) if group_depth is None else (counts, tally, group_depth)
        if not hasattr(bam, "data_ptr") and not all(isinstance(a, np.ndarray) and a.flags.c_contiguous for a in outs):
            raise ValueError("counts, tally and group_depth must be contiguous arrays (they are added to in place)")
        return self.bam_counts(bam, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq_len, counts, tally,
                               group_of_sample, n_groups, sample_status, group_depth, n_quals=n_quals)

    def bam_counts_bgzf_acc(self, comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s, refseq_len,
                            acc, group_of_sample=None, sample_status=None):
        """bvc_bam_counts_bgzf_acc (include/bvc_bam_counts.h): bam_counts from BGZF blocks still compressed (comp / blocks as
        bam_pileup_bgzf takes them), added into `acc` (a SiteAcc of len(positions) positions) with its n_groups.  Host arrays only.
        Returns (rc, sample_status): rc 0, or BAM_MORE (2) -- nothing is added then.  Raises BvcError for the errors."""
        n, _, shared = self._bgzf_inputs(comp, blocks, bam_bytes, sample_off, sample_end, sample_eof, rid, beg0, end0, min_mapq, positions, rg_s,
                                         np.zeros(0, dtype=np.uint8))
        g = None if group_of_sample is None else _as(group_of_sample, np.uint8)
        if g is not None and len(g) != n:
            raise ValueError("group_of_sample must be [n_samples]")
        sample_status = np.zeros(max(1, n), dtype=np.uint32) if sample_status is None else sample_status
        rc = self._L.bvc_bam_counts_bgzf_acc(self._h, n, *_pointers(shared[:-2], _np_ptr), int(refseq_len), _np_ptr(g) if g is not None and n else None,
                                             acc._h, _np_ptr(sample_status) if n else None)
        if rc not in (0, BAM_MORE):
            self._check(rc)
        return rc, sample_status

    # ---- a cohort in sample chunks: counts that accumulate (include/bvc.h).  `counts` is added to IN PLACE: a uint32 / int32 array of
    # [n_sites, 512] (plain) or [n_sites, n_groups + 1, 512] (groups; slot n_groups = in no group), numpy with the host calls, a tensor
    # on this context's device with the *_device calls (asynchronous on the stream).
    def _counts_call(self, fn, sizes, arrays, counts, device, n_groups=None):
        """fn(ctx, *sizes, *arrays, [n_groups,] counts, flags): the argument order of every bvc_counts_add_* call."""
        if device:
            ok = counts.is_contiguous() and counts.element_size() == 4 and not counts.is_floating_point()
        else:
            ok = isinstance(counts, np.ndarray) and counts.flags.c_contiguous and counts.dtype.kind in "iu" and counts.dtype.itemsize == 4
        if not ok:
            raise ValueError("counts must be a contiguous array of 4-byte integers (it is added to in place)")
        groups = () if n_groups is None else (int(n_groups),)
        self._call(fn, device, (*sizes, *arrays, *groups, counts))
        return counts

    def counts_add_dense(self, bases, quals, counts):
        b, q = _as(bases, np.int8), _as(quals, np.int8)
        return self._counts_call(self._L.bvc_counts_add_dense, (b.shape[0], b.shape[1], b.shape[1]), (b, q), counts, False)

    def counts_add_dense_device(self, bases_t, quals_t, counts_t):
        return self._counts_call(self._L.bvc_counts_add_dense, _tile(bases_t, quals_t), (bases_t, quals_t), counts_t, True)

    def counts_add_dense_packed(self, packed, counts):
        p = _as(packed, np.uint8)
        return self._counts_call(self._L.bvc_counts_add_dense_packed, (p.shape[0], p.shape[1], p.shape[1]), (p,), counts, False)

    def counts_add_dense_packed_device(self, packed_t, counts_t):
        return self._counts_call(self._L.bvc_counts_add_dense_packed, _tile(packed_t), (packed_t,), counts_t, True)

    def counts_add_csr(self, offsets, bases, quals, counts):
        o, b, q = _as(offsets, np.int64), _as(bases, np.int8), _as(quals, np.int8)
        return self._counts_call(self._L.bvc_counts_add_csr, (len(o) - 1,), (o, b, q), counts, False)

    def counts_add_csr_device(self, offsets_t, bases_t, quals_t, counts_t):
        return self._counts_call(self._L.bvc_counts_add_csr, (offsets_t.numel() - 1,), (offsets_t, bases_t, quals_t), counts_t, True)

    def counts_add_csr_packed(self, offsets, packed, counts):
        o, p = _as(offsets, np.int64), _as(packed, np.uint8)
        return self._counts_call(self._L.bvc_counts_add_csr_packed, (len(o) - 1,), (o, p), counts, False)

    def counts_add_csr_packed_device(self, offsets_t, packed_t, counts_t):
        return self._counts_call(self._L.bvc_counts_add_csr_packed, (offsets_t.numel() - 1,), (offsets_t, packed_t), counts_t, True)

    def counts_add_dense_groups(self, bases, quals, group_of_sample, n_groups, grp_counts):
        b, q, g = _as(bases, np.int8), _as(quals, np.int8), _as(group_of_sample, np.uint8)
        if g.shape != (b.shape[1],):
            raise ValueError("group_of_sample must have one label per column of the chunk")
        return self._counts_call(self._L.bvc_counts_add_dense_groups, (b.shape[0], b.shape[1], b.shape[1]), (b, q, g), grp_counts, False, n_groups)

    def counts_add_dense_groups_device(self, bases_t, quals_t, group_t, n_groups, grp_counts_t):
        sizes = _tile(bases_t, quals_t)
        assert group_t.numel() == sizes[1]
        return self._counts_call(self._L.bvc_counts_add_dense_groups, sizes, (bases_t, quals_t, group_t), grp_counts_t, True,
                                 n_groups)

    def counts_add_csr_group_labels(self, offsets, bases, quals, group_of_obs, n_groups, grp_counts):
        o, b, q, g = _as(offsets, np.int64), _as(bases, np.int8), _as(quals, np.int8), _as(group_of_obs, np.uint8)
        return self._counts_call(self._L.bvc_counts_add_csr_group_labels, (len(o) - 1,), (o, b, q, g), grp_counts, False, n_groups)

    def counts_add_csr_group_labels_device(self, offsets_t, bases_t, quals_t, group_of_obs_t, n_groups, grp_counts_t):
        return self._counts_call(self._L.bvc_counts_add_csr_group_labels, (offsets_t.numel() - 1,), (offsets_t, bases_t, quals_t, group_of_obs_t),
                                 grp_counts_t, True, n_groups)

    def counts_merge(self, dst, src):
        """dst += src (mod 2^32), numpy arrays of equal size; dst in place."""
        s_ = np.ascontiguousarray(src).view(np.uint32)
        if s_.size != dst.size:
            raise ValueError("dst and src differ in size")
        return self._merge(dst, s_, False)

    def counts_merge_device(self, dst_t, src_t):
        assert dst_t.numel() == src_t.numel() and dst_t.is_contiguous() and src_t.is_contiguous()
        return self._merge(dst_t, src_t, True)

    def _merge(self, dst, src, device):
        self._call(self._L.bvc_counts_merge, device, (int(dst.numel() if device else dst.size), dst, src))
        return dst

    def _lrt_hist_groups(self, device, ns, c, r, min_af, n_groups, res=None, gres=None):
        return tuple(self._call(self._L.bvc_lrt_hist_groups, device, (ns, c, r, float(min_af), int(n_groups)),
                                [(res, (ns,), SITE_DTYPE), (gres, (ns, n_groups), GROUP_DTYPE)]))

    def lrt_hist_groups(self, grp_counts, ref_base, min_af, n_groups):
        """Stage 2 of the group calls on accumulated group histograms [n_sites, n_groups + 1, 512]: (site records, group records)."""
        c = np.ascontiguousarray(grp_counts).view(np.uint32).reshape(-1, n_groups + 1, NCLASS)
        return self._lrt_hist_groups(False, c.shape[0], c, _as(ref_base, np.int8), min_af, n_groups)

    def lrt_hist_groups_device(self, grp_counts_t, ref_t, min_af, n_groups, results_t=None, grp_results_t=None):
        ns = ref_t.numel()
        assert grp_counts_t.numel() == ns * (n_groups + 1) * NCLASS and grp_counts_t.is_contiguous()
        return self._lrt_hist_groups(True, ns, grp_counts_t, ref_t, min_af, n_groups, results_t, grp_results_t)


class Store:
    """One bvc_store (include/bvc_store.h): the binary temp-batch records of n_batches batches of n_positions positions each, kept in the
    memory of one device.  Filled through any contexts of that device (put, Context.bam_pileup_bgzf_store; different batches may be put
    from different threads at once), sealed, then read by Context.pileup_begin_store."""

    def __init__(self, device, n_positions, n_batches, byte_budget=0):
        self._L = load_library()
        h = C.c_void_p()
        rc = self._L.bvc_store_create(C.byref(h), int(device), int(n_positions), int(n_batches), int(byte_budget))
        if rc != 0:
            raise BvcError(f"bvc_store_create(device={device}) failed with code {rc}")
        self._h = h
        self.device, self.n_positions, self.n_batches = int(device), int(n_positions), int(n_batches)

    create = classmethod(lambda cls, *a, **kw: cls(*a, **kw))

    def close(self):
        if getattr(self, "_h", None):
            self._L.bvc_store_destroy(self._h)
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

    def put(self, ctx, batch, n_in_batch, records, rec_start):
        """bvc_store_put: records (bytes or uint8 array) and rec_start (uint32 [n_positions + 1]) of batch `batch` from host memory."""
        buf = np.frombuffer(bytes(records), dtype=np.uint8) if not isinstance(records, np.ndarray) else _as(records, np.uint8)
        rs = _as(rec_start, np.uint32)
        if rs.shape != (self.n_positions + 1,):
            raise ValueError("rec_start must be [n_positions + 1]")
        ctx._check(self._L.bvc_store_put(ctx._h, self._h, int(batch), int(n_in_batch), _np_ptr(buf) if len(buf) else None, len(buf), _np_ptr(rs)))

    def get(self, ctx, batch):
        """bvc_store_get: (records as bytes, rec_start uint32 [n_positions + 1]) of a kept batch."""
        need = C.c_int64(0)
        ctx._check(self._L.bvc_store_get(ctx._h, self._h, int(batch), None, 0, C.byref(need), None))
        records = np.zeros(max(1, need.value), dtype=np.uint8)
        rs = np.zeros(self.n_positions + 1, dtype=np.uint32)
        ctx._check(self._L.bvc_store_get(ctx._h, self._h, int(batch), _np_ptr(records), need.value, C.byref(need), _np_ptr(rs)))
        return records[:need.value].tobytes(), rs

    def seal(self, ctx):
        ctx._check(self._L.bvc_store_seal(ctx._h, self._h))

    def tile(self, t0, max_positions, max_bytes):
        """bvc_store_tile: (n_positions, bytes) of the largest tile from t0 on that the two limits admit; raises ValueError where the
        library refuses (a store that is not sealed, t0 outside it, max_positions < 1)."""
        T, nbytes = C.c_int32(0), C.c_int64(0)
        rc = self._L.bvc_store_tile(self._h, int(t0), int(max_positions), int(max_bytes), C.byref(T), C.byref(nbytes))
        if rc != 0:
            raise ValueError(f"bvc_store_tile refused (code {rc})")
        return T.value, nbytes.value

    def bytes(self):
        """bvc_store_bytes: (used, budget)."""
        used, budget = C.c_int64(0), C.c_int64(0)
        self._L.bvc_store_bytes(self._h, C.byref(used), C.byref(budget))
        return used.value, budget.value


class SiteAcc:
    """One bvc_site_acc (include/bvc_bam_counts.h): class counts [n_positions, slots, 512] and tallies [n_positions] kept in the memory of
    one device, zeroed.  Added to through any contexts of that device (Context.bam_counts_bgzf_acc; several threads may add at once), read
    with get, called where it lies with lrt."""

    def __init__(self, device, n_positions, n_groups=0, byte_budget=0, depth_groups=0, n_quals=None):
        """depth_groups > 0: the second kind (bvc_site_acc_create_depth, include/bvc_bam_group_depth.h) -- one slot of counts, the tallies
        and the depths [n_positions, depth_groups, 4] of that many groups; n_groups must then be 0.  n_quals: the third kind
        (bvc_site_acc_create_quals, include/bvc_site_acc_quals.h) -- one slot of narrow rows [4, n_quals], the tallies and the depths of
        depth_groups groups (0: none); n_groups must be 0."""
        self._L = load_library()
        h = C.c_void_p()
        if (depth_groups or n_quals is not None) and n_groups:
            raise ValueError("an accumulator keeps a slot per group (n_groups) or the groups' depths (depth_groups), not both")
        if n_quals is not None:
            what = f"bvc_site_acc_create_quals(device={device}, n_positions={n_positions}, n_groups={depth_groups}, n_quals={n_quals})"
            rc = self._L.bvc_site_acc_create_quals(C.byref(h), int(device), int(n_positions), int(depth_groups), int(n_quals), int(byte_budget))
        elif depth_groups:
            what = f"bvc_site_acc_create_depth(device={device}, n_positions={n_positions}, n_groups={depth_groups})"
            rc = self._L.bvc_site_acc_create_depth(C.byref(h), int(device), int(n_positions), int(depth_groups), int(byte_budget))
        else:
            what = f"bvc_site_acc_create(device={device}, n_positions={n_positions}, n_groups={n_groups})"
            rc = self._L.bvc_site_acc_create(C.byref(h), int(device), int(n_positions), int(n_groups), int(byte_budget))
        if rc != 0:
            err = BvcError(f"{what} failed with code {rc}")
            err.status = rc
            raise err
        self._h = h
        self.device, self.n_positions, self.n_groups, self.depth_groups = int(device), int(n_positions), int(n_groups), int(depth_groups)
        self.slots = self.n_groups + 1 if self.n_groups else 1
        q = C.c_int32(0)
        self._L.bvc_site_acc_quals(self._h, C.byref(q))
        self.n_quals = q.value                       # the quality columns stored for each base: 128 unless made by create_quals

    create = classmethod(lambda cls, *a, **kw: cls(*a, **kw))
    create_depth = classmethod(lambda cls, device, n_positions, n_groups, byte_budget=0: cls(device, n_positions, 0, byte_budget, depth_groups=n_groups))
    create_quals = classmethod(lambda cls, device, n_positions, n_quals, n_groups=0, byte_budget=0:
                               cls(device, n_positions, 0, byte_budget, depth_groups=n_groups, n_quals=n_quals))

    def close(self):
        if getattr(self, "_h", None):
            self._L.bvc_site_acc_destroy(self._h)
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

    def bytes(self):
        """bvc_site_acc_bytes: (used, budget)."""
        used, budget = C.c_int64(0), C.c_int64(0)
        self._L.bvc_site_acc_bytes(self._h, C.byref(used), C.byref(budget))
        return used.value, budget.value

    def get(self, ctx, t0=0, n=None, counts=True):
        """bvc_site_acc_get: (counts uint32 [n, 512] or [n, n_groups + 1, 512] -- None with counts=False --, tally TALLY_DTYPE [n]) of rows
        [t0, t0 + n)."""
        n = self.n_positions - int(t0) if n is None else int(n)
        shape = (max(n, 0), NCLASS) if not self.n_groups else (max(n, 0), self.slots, NCLASS)
        c = np.zeros(shape, dtype=np.uint32) if counts else None
        t = np.zeros(max(n, 0), dtype=TALLY_DTYPE)
        ctx._check(self._L.bvc_site_acc_get(ctx._h, self._h, int(t0), n, _np_ptr(c) if counts and n > 0 else None, _np_ptr(t) if n > 0 else None))
        return c, t

    def get_depth(self, ctx, t0=0, n=None):
        """bvc_site_acc_get_depth: the groups' depths uint32 [n, depth_groups, 4] of rows [t0, t0 + n); an accumulator of the first kind is
        refused (BVC_ERR_ARG)."""
        n = self.n_positions - int(t0) if n is None else int(n)
        d = np.zeros((max(n, 0), max(self.depth_groups, 1), 4), dtype=np.uint32)
        ctx._check(self._L.bvc_site_acc_get_depth(ctx._h, self._h, int(t0), n, _np_ptr(d) if n > 0 else None))
        return d

    def row_words(self):
        """bvc_site_acc_row_words: (W, slots, depth_groups) of the logical row (include/bvc_site_acc_pack.h)."""
        w, sl, dg = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        rc = self._L.bvc_site_acc_row_words(self._h, C.byref(w), C.byref(sl), C.byref(dg))
        if rc != 0:
            raise BvcError(f"bvc_site_acc_row_words failed with code {rc}")
        return w.value, sl.value, dg.value

    def pack(self, ctx, t0=0, n=None):
        """bvc_site_acc_pack, both steps: (row_start int64 [n + 1], cell uint16 [n_entries], count uint32 [n_entries]) of rows [t0, t0 + n)."""
        n = self.n_positions - int(t0) if n is None else int(n)
        rs = np.zeros(max(n, 0) + 1, dtype=np.int64)
        need = C.c_int64(0)
        rc = self._L.bvc_site_acc_pack(ctx._h, self._h, int(t0), n, _np_ptr(rs), None, None, 0, C.byref(need), BVC_PTR_HOST)
        if rc not in (0, ACC_MORE):
            ctx._check(rc)
        cell, count = np.zeros(need.value, dtype=np.uint16), np.zeros(need.value, dtype=np.uint32)
        if rc == ACC_MORE:
            ctx._check(self._L.bvc_site_acc_pack(ctx._h, self._h, int(t0), n, _np_ptr(rs), _np_ptr(cell), _np_ptr(count), need.value, C.byref(need),
                                                 BVC_PTR_HOST))
        return rs, cell, count

    def add_packed(self, ctx, row_start, cell, count, t0=0):
        """bvc_site_acc_add_packed: the piece (row_start [n + 1], cell, count) ADDED into rows [t0, t0 + n)."""
        rs, ce, co = _as(row_start, np.int64), _as(cell, np.uint16), _as(count, np.uint32)
        if len(rs) < 1 or len(ce) != len(co):
            raise ValueError("row_start must be [n + 1], and cell and count of one length")
        ctx._check(self._L.bvc_site_acc_add_packed(ctx._h, self._h, int(t0), len(rs) - 1, _np_ptr(rs), _np_ptr(ce) if len(ce) else None,
                                                   _np_ptr(co) if len(co) else None, len(ce), BVC_PTR_HOST))

    def lrt(self, ctx, ref_base, min_af, t0=0):
        """bvc_site_acc_lrt: stage 2 on rows [t0, t0 + len(ref_base)) where they lie.  Returns the site records (SITE_DTYPE), or with
        groups (site records, group records [n, n_groups])."""
        r = _as(ref_base, np.int8)
        n = len(r)
        res = np.zeros(n, dtype=SITE_DTYPE)
        gres = np.zeros((n, self.n_groups), dtype=GROUP_DTYPE) if self.n_groups else None
        ctx._check(self._L.bvc_site_acc_lrt(ctx._h, self._h, int(t0), n, _np_ptr(r) if n else None, float(min_af), _np_ptr(res) if n else None,
                                            _np_ptr(gres) if gres is not None and n else None))
        return (res, gres) if self.n_groups else res


def results_from_tensor(results_t):
    """uint8 CUDA/CPU tensor of packed bvc_site_result -> numpy structured array (synchronises)."""
    return results_t.cpu().numpy().view(SITE_DTYPE)
