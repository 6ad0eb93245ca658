"""ctypes binding of the C ABI declared in include/glrm_hip.h.

The product binds ``libglrm_hip.so`` with the ``glrm_hip_`` prefix (:func:`hip_api`).  The
same binder is reused by tests/ to bind the CPU oracle (``glrm_cpu_`` prefix) -- the product
never does that, and :func:`hip_api` raises if the HIP library is missing (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

ABI_VERSION = 3

GLRM_OK = 0
ERR_INVALID, ERR_UNSUPPORTED, ERR_HIP, ERR_COMM, ERR_OOM, ERR_NONFINITE = -1, -2, -3, -4, -5, -6
PROBLEM_DEVICE_ARRAYS = 1
PROBLEM_DEFER_SETUP = 2
PROBLEM_BORROW_DEVICE_ARRAYS = 4
PROBLEM_ROWS_FROM_COLS = 8   # Omega is a sparse matrix's pattern: hand over the column view only, the engine derives the row view
SCALE_EQUILIBRATE, SCALE_PROB = 0, 1   # include/glrm_hip_scale.h: equilibrate_variance! / prob_scale!


class GLRMError(RuntimeError):
    """A negative glrm_status from the engine (the reference throws Julia exceptions instead)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"[glrm status {code}] {message}")
        self.code = code
        self.message = message


class CLoss(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dim", C.c_int32), ("scale", C.c_double), ("p0", C.c_double), ("p1", C.c_double)]


class CReg(C.Structure):
    _fields_ = [("kind", C.c_int32), ("wrap", C.c_int32), ("scale", C.c_double)]


LOSS_DTYPE = np.dtype([("kind", "<i4"), ("dim", "<i4"), ("scale", "<f8"), ("p0", "<f8"), ("p1", "<f8")])
REG_DTYPE = np.dtype([("kind", "<i4"), ("wrap", "<i4"), ("scale", "<f8")])
DOMAIN_DTYPE = np.dtype([("kind", "<i4"), ("reserved", "<i4"), ("lo", "<f8"), ("hi", "<f8")])  # glrm_domain, 24 bytes
assert LOSS_DTYPE.itemsize == C.sizeof(CLoss) == 32 and REG_DTYPE.itemsize == C.sizeof(CReg) == 16


class CRegVec(C.Structure):
    """glrm_regvec (include/glrm_hip_regvec.h): one side's vectors, a k x count column-major table and one int32 length per descriptor."""
    _fields_ = [("vec", C.c_void_p), ("len", C.c_void_p)]


class CProblem(C.Structure):
    _fields_ = [
        ("m", C.c_int64), ("n", C.c_int64), ("k", C.c_int32), ("flags", C.c_int32),
        ("row_begin", C.c_int64), ("row_end", C.c_int64), ("col_begin", C.c_int64), ("col_end", C.c_int64),
        ("rowptr", C.c_void_p), ("colidx", C.c_void_p), ("rowvals", C.c_void_p),
        ("colptr", C.c_void_p), ("rowidx", C.c_void_p), ("colvals", C.c_void_p),
        ("losses", C.c_void_p), ("n_losses", C.c_int64),
        ("rx", C.c_void_p), ("n_rx", C.c_int64),
        ("ry", C.c_void_p), ("n_ry", C.c_int64),
        ("dense_A", C.c_void_p), ("dense_ld", C.c_int64), ("dense_colmajor", C.c_int32), ("dense_reserved", C.c_int32),
    ]


class CParams(C.Structure):
    _fields_ = [
        ("stepsize", C.c_double), ("max_iter", C.c_int64), ("inner_iter_X", C.c_int64), ("inner_iter_Y", C.c_int64),
        ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("min_stepsize", C.c_double),
    ]


class CSparseParams(C.Structure):
    _fields_ = [("stepsize", C.c_double), ("max_iter", C.c_int64), ("inner_iter", C.c_int64), ("abs_tol", C.c_double),
                ("min_stepsize", C.c_double)]


class COptions(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("profile", C.c_int32), ("waves_row", C.c_int32), ("waves_col", C.c_int32),
                ("stream", C.c_void_p), ("caller_stream", C.c_int32), ("tiled", C.c_int32), ("quad_gram", C.c_int32),
                ("sum_order", C.c_int32), ("storage", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(COptions) == 48 and COptions.storage.offset == 40
STORAGE_F64, STORAGE_F32 = 0, 1   # include/glrm_hip_storage.h: glrm_options.storage


class CArrival(C.Structure):
    """glrm_arrival: rows [begin, end) of X are complete on the device once ``event`` (a hipEvent_t, 0 = already there) has fired."""
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("event", C.c_void_p)]


class CSignature(C.Structure):
    """glrm_signature: what the kernel choice reads from the WHOLE problem (sum the counts over shards, max the rest)."""
    _fields_ = [("nnz_rows", C.c_int64), ("nnz_cols", C.c_int64), ("max_row_len", C.c_int64), ("max_col_len", C.c_int64),
                ("rows_unordered", C.c_int32), ("cols_unordered", C.c_int32)]
    SUM_FIELDS = ("nnz_rows", "nnz_cols")

    def astuple(self):
        return tuple(int(getattr(self, f)) for f, _ in self._fields_)

    @classmethod
    def combine(cls, parts):
        """The whole problem's signature from the shards' (each a CSignature or its astuple())."""
        parts = [p.astuple() if isinstance(p, cls) else tuple(int(v) for v in p) for p in parts]
        out = cls()
        for i, (f, _) in enumerate(cls._fields_):
            vals = [p[i] for p in parts]
            setattr(out, f, sum(vals) if f in cls.SUM_FIELDS else max(vals))
        return out


class CMultiOptions(C.Structure):
    _fields_ = [("n_shards", C.c_int32), ("exchange", C.c_int32), ("device_ids", C.c_void_p), ("x_chunks", C.c_int32), ("arrival", C.c_int32)]


class CKernelStats(C.Structure):
    _fields_ = [
        ("launches_x", C.c_int64), ("launches_y", C.c_int64), ("ms_x", C.c_double), ("ms_y", C.c_double),
        ("trials_x", C.c_int64), ("trials_y", C.c_int64), ("accepts_x", C.c_int64), ("accepts_y", C.c_int64),
        ("nnz_rows", C.c_int64), ("nnz_cols", C.c_int64),
        ("waves_row", C.c_int32), ("waves_col", C.c_int32), ("ld", C.c_int32), ("tiled", C.c_int32),
        ("ms_wait_y", C.c_double),
    ]

    def asdict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class CSumOrder(C.Structure):
    """glrm_sum_order: the order in which a handle adds the terms of a segment's sums (include/glrm_hip.h)."""
    _fields_ = [("family", C.c_int32), ("lanes", C.c_int32), ("comps", C.c_int32), ("waves", C.c_int32),
                ("waves4_from", C.c_int64), ("waves8_from", C.c_int64), ("cached_maxlen", C.c_int64),
                ("cached_waves", C.c_int32), ("batch", C.c_int32), ("batch_one_wave_only", C.c_int32), ("rotate", C.c_int32),
                ("window", C.c_int64), ("windows_per_sup", C.c_int64), ("private_order", C.c_int32), ("long_from", C.c_int32)]
    FAMILIES = {0: "reference", 1: "strided", 2: "windowed", 3: "other"}

    def asdict(self):
        d = {f: int(getattr(self, f)) for f, _ in self._fields_}
        d["family_name"] = self.FAMILIES.get(d["family"], "?")
        return d


assert C.sizeof(CSumOrder) == 80

#: every symbol include/glrm_hip.h declares (suffix after the prefix); the CPU test-suite checks
#: that the built library exports all of them.
ABI_SYMBOLS = (
    "version", "last_error", "create", "destroy", "signature", "finalize", "fit", "fit_sparse", "objective", "factor_ld", "bind_buffers",
    "set_factors", "get_factors", "reset_stepsizes", "step_x", "step_y", "step_y_arrival", "step_x_range", "gradstep_x", "gradstep_y", "col_losses", "row_penalties",
    "col_penalties", "set_regularizers", "subset", "init_svd", "error_metric", "impute", "sum", "synchronize", "kernel_stats", "sum_order",
    "multi_create", "multi_fit", "multi_set_regularizers", "multi_info", "multi_destroy",
)

#: the scaling extension, include/glrm_hip_scale.h: NOT part of the 37-symbol boundary above, bound only where the library has it
#: (the HIP engine; the CPU oracle does not restate it)
SCALE_SYMBOLS = ("scale_columns",)

#: the initialization extension, include/glrm_hip_init.h: outside the boundary as well, bound only where the library has it
INIT_SYMBOLS = ("init_kmeanspp",)

#: the storage extension, include/glrm_hip_storage.h (fp32 storage of A, X and Y): outside the boundary, bound only where the library has it
STORAGE_SYMBOLS = ("storage",)

#: the vector-carrying regularizers, include/glrm_hip_regvec.h: outside the boundary, bound only where the library has them
REGVEC_SYMBOLS = ("set_regularizers_vec", "multi_set_regularizers_vec")

#: the top-k extension, include/glrm_hip_topk.h (the rank-th largest entry of X'Y, the ordered scan of precision_at_k): outside the boundary,
#: bound only where the library has it
TOPK_SYMBOLS = ("xy_select", "xy_select_info", "precision_scan")

#: the recommend extension, include/glrm_hip_recommend.h (the kper best columns of every queried row of X'Y, observed ones left out):
#: outside the boundary, bound only where the library has it
RECOMMEND_SYMBOLS = ("row_topk", "row_topk_info")
ROW_TOPK_MAX = 128   # glrm_hip_recommend.h: GLRM_ROW_TOPK_MAX

#: the NMF initialization extension, include/glrm_hip_nmf.h (init_nndsvd! on the resident lists): outside the boundary, bound only where
#: the library has it
NMF_SYMBOLS = ("init_nndsvd",)
NNDSVD_VARIANTS = {"std": 0, "a": 1, "ar": 2}   # glrm_hip_nmf.h: GLRM_NNDSVD_STD / _A / _AR (ar is refused)

#: the transform extension, include/glrm_hip_transform.h (inner_iter X half-steps against a fixed Y, fused into one launch where the
#: register kernel admits the rows): outside the boundary, bound only where the library has it
TRANSFORM_SYMBOLS = ("solve_x", "solve_x_info")

#: the impute_at extension, include/glrm_hip_impute_at.h (imputed values and errors at listed entries, whole rows or whole columns, nothing
#: m x n): outside the boundary, bound only where the library has it
IMPUTE_AT_SYMBOLS = ("impute_at", "impute_at_info")
IMPUTE_AT_PAIRS, IMPUTE_AT_ROWS, IMPUTE_AT_COLS = 0, 1, 2   # glrm_hip_impute_at.h: GLRM_IMPUTE_AT_*

#: the sampling extension, include/glrm_hip_sample.h (draws from the fitted model at listed entries, whole rows or whole columns, nothing
#: m x n): outside the boundary, bound only where the library has it
SAMPLE_SYMBOLS = ("sample_at", "sample_at_info")
SAMPLE_NOISE = {"residual": 0, "reference": 1, "given": 2}   # glrm_hip_sample.h: GLRM_SAMPLE_NOISE_*

#: the ALS extension, include/glrm_hip_als.h (the exact half-step of a QuadLoss + QuadReg / ZeroReg model: one Gram matrix and one
#: rank-k Cholesky per row or column): outside the boundary, bound only where the library has it
ALS_SYMBOLS = ("als_solve", "als_info")
ALS_MAX_K = 64                                         # glrm_hip_als.h: GLRM_ALS_MAX_K
ALS_SOLVED, ALS_KEPT_SHORT, ALS_KEPT_PIVOT = 0, 1, 2   # glrm_hip_als.h: GLRM_ALS_*

#: the coordinate-descent extension, include/glrm_hip_cd.h (cyclic coordinate-descent sweeps on every row or column of a QuadLoss model
#: with ZeroReg / QuadReg / OneReg / NonNegConstraint on the solved side): outside the boundary, bound only where the library has it
CD_SYMBOLS = ("cd_solve", "cd_info")
CD_MAX_K, CD_MAX_SWEEPS = 64, 256                      # glrm_hip_cd.h: GLRM_CD_MAX_K, GLRM_CD_MAX_SWEEPS
CD_CONVERGED, CD_SKIPPED = 1, 2                        # glrm_hip_cd.h: GLRM_CD_* status bits

#: the streaming extension, include/glrm_hip_stream.h (the reference's one-pass streaming_fit! on the device: rows run level by level, the
#: decay of Y is applied when a column is read): outside the boundary, bound only where the library has it
STREAM_SYMBOLS = ("stream_plan", "stream_rows", "stream_info")
STREAM_MAX_K = 64                                      # glrm_hip_stream.h: GLRM_STREAM_MAX_K


#: Bumped whenever a loss / regularizer object is created or modified or a model's descriptor list changes: lets a model reuse
#: its packed descriptors (and its engine handle) without re-reading a million Python objects per fit! call.
EPOCH = [0]


def bump_epoch():
    EPOCH[0] += 1


class TrackedList(list):
    """A list whose mutations bump EPOCH (the losses / rx / ry lists of a GLRM)."""

    def _mut(name):  # noqa: N805
        base = getattr(list, name)

        def f(self, *a, **k):
            bump_epoch()
            return base(self, *a, **k)
        f.__name__ = name
        return f

    for _n in ("__setitem__", "__delitem__", "__iadd__", "__imul__", "append", "extend", "insert", "pop", "remove", "clear", "sort", "reverse"):
        locals()[_n] = _mut(_n)
    del _n, _mut


def _ptr(a):
    """numpy array -> address; int -> address; None -> NULL."""
    if a is None:
        return None
    if isinstance(a, (int, np.integer)):
        return int(a)
    return a.ctypes.data


class Api:
    """One loaded library + symbol prefix.  Thin, stateless, no numerics."""

    def __init__(self, lib: C.CDLL, prefix: str, device_type: str):
        self.lib, self.prefix, self.device_type = lib, prefix, device_type
        self.dense_ok = prefix == "glrm_hip_"  # the dense (matrix-core) hand-over exists in the HIP engine only
        H = C.c_void_p
        sig = {
            "version": (C.c_int, []),
            "last_error": (C.c_char_p, []),
            "create": (C.c_int, [C.POINTER(H), C.POINTER(CProblem), C.POINTER(COptions)]),
            "destroy": (None, [H]),
            "signature": (C.c_int, [H, C.POINTER(CSignature)]),
            "finalize": (C.c_int, [H, C.POINTER(CSignature)]),
            "fit": (C.c_int, [H, C.POINTER(CParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                              C.POINTER(C.c_int64)]),
            "fit_sparse": (C.c_int, [H, C.POINTER(CSparseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_int64)]),
            "gradstep_x": (C.c_int, [H, C.c_double]),
            "gradstep_y": (C.c_int, [H, C.c_double]),
            "objective": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
            "factor_ld": (C.c_int, [H]),
            "bind_buffers": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            "set_factors": (C.c_int, [H, C.c_void_p, C.c_void_p]),
            "get_factors": (C.c_int, [H, C.c_void_p, C.c_void_p]),
            "reset_stepsizes": (C.c_int, [H, C.c_double]),
            "step_x": (C.c_int, [H, C.c_double]),
            "step_y": (C.c_int, [H, C.c_double]),
            "step_y_arrival": (C.c_int, [H, C.c_double, C.c_void_p, C.c_int32]),
            "step_x_range": (C.c_int, [H, C.c_int64, C.c_int64, C.c_double]),
            "col_losses": (C.c_int, [H]),
            "row_penalties": (C.c_int, [H]),
            "col_penalties": (C.c_int, [H]),
            "set_regularizers": (C.c_int, [H, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
            "subset": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(H)]),
            "init_svd": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_uint64, C.c_void_p, C.POINTER(C.c_int32)]),
            "error_metric": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_double)]),
            "impute": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            "sum": (C.c_int, [H, C.c_void_p, C.c_int64, C.POINTER(C.c_double)]),
            "synchronize": (C.c_int, [H]),
            "kernel_stats": (C.c_int, [H, C.POINTER(CKernelStats), C.c_int]),
            "sum_order": (C.c_int, [H, C.c_int32, C.POINTER(CSumOrder)]),
            "multi_create": (C.c_int, [C.POINTER(H), C.POINTER(CProblem), C.POINTER(COptions), C.POINTER(CMultiOptions)]),
            "multi_fit": (C.c_int, [H, C.POINTER(CParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64)]),
            "multi_set_regularizers": (C.c_int, [H, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
            "multi_info": (C.c_int, [H, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
            "multi_destroy": (None, [H]),
        }
        self._f = {}
        for name, (res, args) in sig.items():
            fn = getattr(lib, prefix + name)
            fn.restype, fn.argtypes = res, args
            self._f[name] = fn
        ext = {
            "scale_columns": (C.c_int, [C.POINTER(CProblem), C.POINTER(COptions), C.c_int32] + [C.c_void_p] * 5),
            "init_kmeanspp": (C.c_int, [H, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
            "storage": (C.c_int, [H]),
            "set_regularizers_vec": (C.c_int, [H, C.c_void_p, C.c_int64, C.POINTER(CRegVec), C.c_void_p, C.c_int64, C.POINTER(CRegVec)]),
            "multi_set_regularizers_vec": (C.c_int, [H, C.c_void_p, C.c_int64, C.POINTER(CRegVec), C.c_void_p, C.c_int64, C.POINTER(CRegVec)]),
            "xy_select": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
            "xy_select_info": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
            "precision_scan": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
            "row_topk": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
            "row_topk_info": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
            "init_nndsvd": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
            "solve_x": (C.c_int, [H, C.c_int64, C.c_double]),
            "solve_x_info": (C.c_int, [H, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
            "impute_at": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
            "impute_at_info": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
            "sample_at": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_int32,
                                    C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
            "sample_at_info": (C.c_int, [C.POINTER(C.c_int64)] * 5),
            "als_solve": (C.c_int, [H, C.c_int32]),
            "als_info": (C.c_int, [H, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]),
            "cd_solve": (C.c_int, [H, C.c_int32, C.c_int32]),
            "cd_info": (C.c_int, [H, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]),
            "stream_plan": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
                            + [C.POINTER(C.c_int64)] * 4),
            "stream_rows": (C.c_int, [H, C.c_int64, C.c_double, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            "stream_info": (C.c_int, [H] + [C.POINTER(C.c_int64)] * 6 + [C.POINTER(C.c_double), C.c_void_p]),
        }
        assert tuple(ext) == (SCALE_SYMBOLS + INIT_SYMBOLS + STORAGE_SYMBOLS + REGVEC_SYMBOLS + TOPK_SYMBOLS + RECOMMEND_SYMBOLS + NMF_SYMBOLS + TRANSFORM_SYMBOLS
                              + IMPUTE_AT_SYMBOLS + SAMPLE_SYMBOLS + ALS_SYMBOLS + CD_SYMBOLS + STREAM_SYMBOLS)
        for name, (res, args) in ext.items():
            fn = getattr(lib, prefix + name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
                self._f[name] = fn
        v = self._f["version"]()
        if v != ABI_VERSION:
            raise RuntimeError(f"{prefix}version() = {v}, this host layer speaks ABI {ABI_VERSION}")

    # -- error plumbing ---------------------------------------------------------------
    def last_error(self) -> str:
        m = self._f["last_error"]()
        return m.decode("utf-8", "replace") if m else ""

    def _ck(self, rc: int):
        if rc != GLRM_OK:
            raise GLRMError(rc, self.last_error())

    # -- lifecycle --------------------------------------------------------------------
    @staticmethod
    def _cproblem(prob):
        p = CProblem()
        p.m, p.n, p.k, p.flags = prob.m, prob.n, prob.k, prob.flags
        p.row_begin, p.row_end, p.col_begin, p.col_end = prob.row_begin, prob.row_end, prob.col_begin, prob.col_end
        p.rowptr, p.colidx, p.rowvals = _ptr(prob.rowptr), _ptr(prob.colidx), _ptr(prob.rowvals)
        p.colptr, p.rowidx, p.colvals = _ptr(prob.colptr), _ptr(prob.rowidx), _ptr(prob.colvals)
        p.losses, p.n_losses = _ptr(prob.losses), len(prob.losses)
        p.rx, p.n_rx = _ptr(prob.rx), len(prob.rx)
        p.ry, p.n_ry = _ptr(prob.ry), len(prob.ry)
        if prob.dense_A is not None:
            p.dense_A, p.dense_ld, p.dense_colmajor, p.dense_reserved = _ptr(prob.dense_A), prob.dense_ld, prob.dense_colmajor, 0
        return p

    def create(self, prob: "ProblemArrays", device_id=-1, profile=0, waves_row=0, waves_col=0, stream=None, tiled=0, quad_gram=0, defer=False,
               sum_order=0, storage=0):
        """``stream=None``: the handle creates a private stream.  ``stream=<int>``: launch on exactly that
        hipStream_t -- 0 is the legacy default stream (what torch.cuda.current_stream().cuda_stream returns
        for the default stream), so kernels stay ordered with the caller's other work on it.
        ``defer=True`` (one shard of a sharded fit): only upload; the host combines :meth:`signature` over the shards and
        calls :meth:`finalize` on every one of them (GLRM_PROBLEM_DEFER_SETUP).
        ``sum_order=1``: the reference-order validation sweeps (glrm_options.sum_order).
        ``storage=1``: A, X and Y stored as floats on the gather sweeps and the cached row sweep, arithmetic in fp64
        (glrm_options.storage, include/glrm_hip_storage.h); the factors cross this boundary as float64 arrays either way."""
        if prob.dense_A is not None and not self.dense_ok:
            raise GLRMError(ERR_UNSUPPORTED, "this engine takes observation lists only")
        p = self._cproblem(prob)
        if defer:
            p.flags |= PROBLEM_DEFER_SETUP
        o = COptions(device_id, profile, waves_row, waves_col, (stream or None), 0 if stream is None else 1, tiled, int(quad_gram), int(sum_order),
                     int(storage), 0)
        h = C.c_void_p()
        self._ck(self._f["create"](C.byref(h), C.byref(p), C.byref(o)))
        return h

    def signature(self, h) -> CSignature:
        sig = CSignature()
        self._ck(self._f["signature"](h, C.byref(sig)))
        return sig

    def finalize(self, h, whole: "CSignature | None" = None):
        self._ck(self._f["finalize"](h, C.byref(whole) if whole is not None else None))

    # -- one process, several devices (glrm_*_multi_*) -----------------------------------------
    def multi_create(self, prob: "ProblemArrays", n_shards, device_ids=None, exchange=0, x_chunks=0, profile=0, waves_row=0,
                     waves_col=0, tiled=0, quad_gram=0, arrival=0, sum_order=0, storage=0):
        """The whole problem (host arrays), sharded by the library over ``device_ids`` (default 0..n_shards-1; ids may repeat)."""
        if prob.dense_A is not None and not self.dense_ok:
            raise GLRMError(ERR_UNSUPPORTED, "this engine takes observation lists only")
        p = self._cproblem(prob)
        o = COptions(-1, profile, waves_row, waves_col, None, 0, tiled, int(quad_gram), int(sum_order), int(storage), 0)  # (storage = 1 is refused)
        ids = None if device_ids is None else np.ascontiguousarray(device_ids, dtype=np.int32)
        if ids is not None and len(ids) != n_shards:
            raise ValueError("device_ids must have n_shards entries")
        mo = CMultiOptions(int(n_shards), int(exchange), _ptr(ids), int(x_chunks), int(arrival))
        h = C.c_void_p()
        self._ck(self._f["multi_create"](C.byref(h), C.byref(p), C.byref(o), C.byref(mo)))
        return h

    def multi_fit(self, mh, params, X, Y):
        cap = int(params.max_iter) + 1
        obj, sec = np.zeros(cap), np.zeros(cap)
        nrec = C.c_int64(0)
        cp = CParams(params.stepsize, params.max_iter, params.inner_iter_X, params.inner_iter_Y, params.abs_tol,
                     params.rel_tol, params.min_stepsize)
        self._ck(self._f["multi_fit"](mh, C.byref(cp), _ptr(X), _ptr(Y), _ptr(obj), _ptr(sec), cap, C.byref(nrec)))
        return obj[: nrec.value].copy(), sec[: nrec.value].copy()

    def multi_set_regularizers(self, mh, rx, ry):
        self._ck(self._f["multi_set_regularizers"](mh, _ptr(rx), len(rx), _ptr(ry), len(ry)))

    def multi_info(self, mh, n_shards):
        rb, cb = np.zeros(n_shards + 1, np.int64), np.zeros(n_shards + 1, np.int64)
        ex, ms = C.c_int32(0), C.c_double(0.0)
        self._ck(self._f["multi_info"](mh, _ptr(rb), _ptr(cb), C.byref(ex), C.byref(ms)))
        return {"row_bounds": rb.tolist(), "col_bounds": cb.tolist(), "exchange": ex.value, "exchange_ms": ms.value}

    def multi_destroy(self, mh):
        if mh is not None and mh.value:
            self._f["multi_destroy"](mh)
            mh.value = None

    def destroy(self, h):
        if h is not None and h.value:
            self._f["destroy"](h)
            h.value = None

    # -- whole-fit --------------------------------------------------------------------
    def fit(self, h, params, X, Y):
        cap = int(params.max_iter) + 1
        obj = np.zeros(cap)
        sec = np.zeros(cap)
        nrec = C.c_int64(0)
        cp = CParams(params.stepsize, params.max_iter, params.inner_iter_X, params.inner_iter_Y, params.abs_tol,
                     params.rel_tol, params.min_stepsize)
        self._ck(self._f["fit"](h, C.byref(cp), _ptr(X), _ptr(Y), _ptr(obj), _ptr(sec), cap, C.byref(nrec)))
        return obj[: nrec.value].copy(), sec[: nrec.value].copy()

    def fit_sparse(self, h, params, X, Y):
        cap = int(params.max_iter) + 2
        obj, sec = np.zeros(cap), np.zeros(cap)
        nrec = C.c_int64(0)
        cp = CSparseParams(params.stepsize, params.max_iter, params.inner_iter, params.abs_tol, params.min_stepsize)
        self._ck(self._f["fit_sparse"](h, C.byref(cp), _ptr(X), _ptr(Y), _ptr(obj), _ptr(sec), cap, C.byref(nrec)))
        return obj[: nrec.value].copy(), sec[: nrec.value].copy()

    def gradstep_x(self, h, alpha):
        self._ck(self._f["gradstep_x"](h, float(alpha)))

    def gradstep_y(self, h, alpha):
        self._ck(self._f["gradstep_y"](h, float(alpha)))

    def objective(self, h, X, Y, include_reg=True) -> float:
        out = C.c_double(0.0)
        self._ck(self._f["objective"](h, _ptr(X), _ptr(Y), 1 if include_reg else 0, C.byref(out)))
        return out.value

    # -- step-level -------------------------------------------------------------------
    def factor_ld(self, h) -> int:
        ld = self._f["factor_ld"](h)
        if ld <= 0:
            raise GLRMError(ld, self.last_error())
        return ld

    def bind_buffers(self, h, dX, dY, dObjCol, dObjRow):
        self._ck(self._f["bind_buffers"](h, _ptr(dX), _ptr(dY), _ptr(dObjCol), _ptr(dObjRow)))

    def set_factors(self, h, X, Y):
        self._ck(self._f["set_factors"](h, _ptr(X), _ptr(Y)))

    def get_factors(self, h, X, Y):
        self._ck(self._f["get_factors"](h, _ptr(X), _ptr(Y)))

    def reset_stepsizes(self, h, stepsize):
        self._ck(self._f["reset_stepsizes"](h, float(stepsize)))

    def step_x(self, h, min_stepsize):
        self._ck(self._f["step_x"](h, float(min_stepsize)))

    def step_x_range(self, h, seg_begin, seg_end, min_stepsize):
        self._ck(self._f["step_x_range"](h, int(seg_begin), int(seg_end), float(min_stepsize)))

    def step_y(self, h, min_stepsize):
        self._ck(self._f["step_y"](h, float(min_stepsize)))

    def step_y_arrival(self, h, min_stepsize, blocks):
        """The Y half-step while X is arriving: ``blocks`` = [(begin, end, event)] tiling the rows [0, m) in the order the host
        expects them; ``event`` is a hipEvent_t as an integer (torch.cuda.Event(...).cuda_event) or 0 / None for rows already there."""
        arr = (CArrival * max(len(blocks), 1))()
        for i, (b, e, ev) in enumerate(blocks):
            arr[i] = CArrival(int(b), int(e), int(ev) if ev else None)
        self._ck(self._f["step_y_arrival"](h, float(min_stepsize), C.cast(arr, C.c_void_p), len(blocks)))

    def col_losses(self, h):
        self._ck(self._f["col_losses"](h))

    def row_penalties(self, h):
        self._ck(self._f["row_penalties"](h))

    def col_penalties(self, h):
        self._ck(self._f["col_penalties"](h))

    def set_regularizers(self, h, rx, ry):
        """rx, ry: REG_DTYPE arrays with the same lengths as at create."""
        self._ck(self._f["set_regularizers"](h, _ptr(rx), len(rx), _ptr(ry), len(ry)))

    # -- vector-carrying regularizers (include/glrm_hip_regvec.h) --------------------------------
    def _set_regs_vec(self, name, h, rx, vx, ry, vy):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the regularizers that carry a vector "
                                             "(include/glrm_hip_regvec.h is implemented by the HIP engine only)")
        keep = []  # the arrays must outlive the call

        def side(v):
            if v is None:
                return None
            vec, lens = np.ascontiguousarray(v[0], dtype=np.float64), np.ascontiguousarray(v[1], dtype=np.int32)
            keep.extend((vec, lens))
            return C.byref(CRegVec(_ptr(vec), _ptr(lens)))
        self._ck(fn(h, _ptr(rx), len(rx), side(vx), _ptr(ry), len(ry), side(vy)))

    def set_regularizers_vec(self, h, rx, vx, ry, vy):
        """glrm_hip_set_regularizers_vec.  rx, ry: REG_DTYPE arrays that may hold the codes of include/glrm_hip_regvec.h; vx, vy: None or
        (flat k x count column-major table, int32 lengths) for the side."""
        self._set_regs_vec("set_regularizers_vec", h, rx, vx, ry, vy)

    def multi_set_regularizers_vec(self, mh, rx, vx, ry, vy):
        self._set_regs_vec("multi_set_regularizers_vec", mh, rx, vx, ry, vy)

    def subset(self, h, row_tags, col_tags, match, invert=False):
        """Child handle over the entries whose tag (uint8 per entry of the parent's row view / column view) equals
        ``match`` (or differs from it when ``invert``): the train / test split of the cross-validation drivers, compacted
        from the parent's resident data.  The child of a SHARD parent (row / column ranges not the whole problem) comes back
        deferred: read ``signature`` of every shard's child, combine (sum the counts, max the rest) and ``finalize`` each child
        with the whole subset problem's signature before the first step-level call (include/glrm_hip.h, glrm_hip_subset)."""
        row_tags = np.ascontiguousarray(row_tags, dtype=np.uint8)
        col_tags = np.ascontiguousarray(col_tags, dtype=np.uint8)
        out = C.c_void_p()
        self._ck(self._f["subset"](h, _ptr(row_tags), _ptr(col_tags), int(match), 1 if invert else 0, C.byref(out)))
        return out

    def init_svd(self, h, X, Y, max_iter=0, tol=0.0, seed=1):
        """init_svd! on the handle's resident lists: fills X (k x m) and Y (k x d); returns (singular values, iterations)."""
        sv = np.zeros(X.shape[0])
        it = C.c_int32(0)
        self._ck(self._f["init_svd"](h, _ptr(X), _ptr(Y), int(max_iter), float(tol), int(seed), _ptr(sv), C.byref(it)))
        return sv, it.value

    def error_metric(self, h, X, Y, domains, standardize=False) -> float:
        """domains: DOMAIN_DTYPE array, one per column."""
        out = C.c_double(0.0)
        self._ck(self._f["error_metric"](h, _ptr(X), _ptr(Y), _ptr(domains), 1 if standardize else 0, C.byref(out)))
        return out.value

    def impute(self, h, X, Y, domains, m, n):
        Ahat = np.zeros((m, n), order="F")
        self._ck(self._f["impute"](h, _ptr(X), _ptr(Y), _ptr(domains), _ptr(Ahat)))
        return Ahat

    def sum(self, h, vec, n) -> float:
        out = C.c_double(0.0)
        self._ck(self._f["sum"](h, _ptr(vec), int(n), C.byref(out)))
        return out.value

    def synchronize(self, h):
        self._ck(self._f["synchronize"](h))

    def kernel_stats(self, h, reset=False) -> dict:
        st = CKernelStats()
        self._ck(self._f["kernel_stats"](h, C.byref(st), 1 if reset else 0))
        return st.asdict()


    def sum_order(self, h, which) -> CSumOrder:
        """which: 0 = row view (X half-step), 1 = column view (Y half-step)."""
        o = CSumOrder()
        self._ck(self._f["sum_order"](h, int(which), C.byref(o)))
        return o

    # -- storage extension (include/glrm_hip_storage.h) -------------------------------------
    def storage(self, h) -> int:
        """glrm_hip_storage: STORAGE_F64 or STORAGE_F32 (an engine without the extension stores fp64)."""
        fn = self._f.get("storage")
        if fn is None:
            return STORAGE_F64
        s = fn(h)
        if s < 0:
            raise GLRMError(s, self.last_error())
        return s

    # -- scaling extension (include/glrm_hip_scale.h) ---------------------------------------
    def scale_columns(self, prob: "ProblemArrays", mode, device_id=-1, stream=None, diagnostics=False, storage=0):
        """glrm_hip_scale_columns on the column view of ``prob`` (its row view may be None): the NEW loss and Y-regularizer scales of the
        columns [col_begin, col_end) under equilibrate_variance! (``SCALE_EQUILIBRATE``) or prob_scale! (``SCALE_PROB``).  Returns
        (loss_scale, ry_scale), with ``diagnostics`` also a dict of the per-column m_est / avg_loss / variance."""
        fn = self._f.get("scale_columns")
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}scale_columns: this engine does not have the scaling extension "
                                             "(include/glrm_hip_scale.h is implemented by the HIP engine only)")
        p = self._cproblem(prob)
        o = COptions(device_id, 0, 0, 0, (stream or None), 0 if stream is None else 1, 0, 0, 0, int(storage), 0)  # (storage = 1 is refused)
        nl = prob.col_end - prob.col_begin
        out = [np.full(max(nl, 1), np.nan) for _ in range(5 if diagnostics else 2)]
        ptrs = [_ptr(x) for x in out] + [None] * (5 - len(out))
        self._ck(fn(C.byref(p), C.byref(o), int(mode), *ptrs))
        out = [x[:nl] for x in out]
        if diagnostics:
            return out[0], out[1], dict(m_est=out[2], avg_loss=out[3], variance=out[4])
        return out[0], out[1]

    # -- initialization extension (include/glrm_hip_init.h) ---------------------------------
    def init_kmeanspp(self, h, Y, first, u, want_weights=False, m=None):
        """glrm_hip_init_kmeanspp on the handle's resident lists.  ``Y``: the randn(k, n) draw, Fortran-ordered float64, overwritten
        with the initialized factor; ``first``: the 0-based first centre; ``u``: the k-1 uniform draws of the rounds.  Returns
        (centers, weights): the k chosen rows and, with ``want_weights`` (which needs ``m``, the rows of the handle's problem), the
        (k-1) x m array of every round's sampling weights (else None)."""
        fn = self._f.get("init_kmeanspp")
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}init_kmeanspp: this engine does not have the initialization extension "
                                             "(include/glrm_hip_init.h is implemented by the HIP engine only)")
        if not (isinstance(Y, np.ndarray) and Y.dtype == np.float64 and Y.ndim == 2 and Y.flags.f_contiguous):
            raise ValueError("Y must be a Fortran-ordered float64 k x n array (it is overwritten in place)")
        k, n = Y.shape
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if len(u) != k - 1:
            raise ValueError(f"u must hold k - 1 = {k - 1} draws, got {len(u)}")
        centers = np.full(k, -1, dtype=np.int64)
        weights = None
        if want_weights:
            if m is None:
                raise ValueError("want_weights needs m, the number of rows of the handle's problem (the buffer is (k-1) x m)")
            weights = np.full((k - 1, int(m)), np.nan)
        self._ck(fn(h, _ptr(Y), int(first), _ptr(u) if k > 1 else None, _ptr(centers), _ptr(weights) if k > 1 else None))
        return centers, weights

    # -- NMF initialization extension (include/glrm_hip_nmf.h) -----------------------------
    def init_nndsvd(self, h, X, Y, scale=True, zeroh=False, variant="std", max_iters=0, svd_max_iter=0, svd_tol=0.0, seed=1):
        """glrm_hip_init_nndsvd on the handle's resident lists: fills ``X`` (k x m) and ``Y`` (k x n), Fortran-ordered float64.  The lists
        must not hold a pair twice (the caller's contract; :func:`initialize.init_nndsvd_` checks it).  Returns a dict: the
        ``singular_values`` of the last round, ``split`` (k x 2: the larger and the smaller of (mp, mn) per component, last round) and
        ``iterations`` (the subspace iterations of each of the max_iters + 1 rounds)."""
        fn = self._f.get("init_nndsvd")
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}init_nndsvd: this engine does not have the NMF initialization extension "
                                             "(include/glrm_hip_nmf.h is implemented by the HIP engine only)")
        if variant not in NNDSVD_VARIANTS:
            raise ValueError(f"variant must be one of {sorted(NNDSVD_VARIANTS)}, got {variant!r}")
        for name, F in (("X", X), ("Y", Y)):
            if not (isinstance(F, np.ndarray) and F.dtype == np.float64 and F.ndim == 2 and F.flags.f_contiguous):
                raise ValueError(f"{name} must be a Fortran-ordered float64 k x count array (it is overwritten in place)")
        k = X.shape[0]
        sv, split = np.zeros(k), np.zeros((k, 2))
        iters = np.zeros(max(int(max_iters), 0) + 1, dtype=np.int32)
        self._ck(fn(h, _ptr(X), _ptr(Y), 1 if scale else 0, 1 if zeroh else 0, NNDSVD_VARIANTS[variant], int(max_iters), int(svd_max_iter),
                    float(svd_tol), int(seed), _ptr(sv), _ptr(split), _ptr(iters)))
        return dict(singular_values=sv, split=split, iterations=iters)

    # -- transform extension (include/glrm_hip_transform.h) ----------------------------------
    def _transform(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the transform extension "
                                             "(include/glrm_hip_transform.h is implemented by the HIP engine only)")
        return fn

    @property
    def has_transform(self) -> bool:
        """The library exports the transform extension (the CPU oracle does not: a host loops ``step_x`` there)."""
        return "solve_x" in self._f

    def solve_x(self, h, inner_iter, min_stepsize):
        """glrm_hip_solve_x: ``inner_iter`` X half-steps of every local row with Y as it stands; the step sizes are not reset."""
        self._ck(self._transform("solve_x")(h, int(inner_iter), float(min_stepsize)))

    def solve_x_info(self, h) -> dict:
        """What the last solve_x on the handle did: ``fused`` (1: rows of at most 104 / 208 observations ran all their steps in one launch
        of the register kernel), ``fused_rows`` and ``loop_rows`` (rows that ran inner_iter sweep launches)."""
        fused, fr, lr = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._ck(self._transform("solve_x_info")(h, C.byref(fused), C.byref(fr), C.byref(lr)))
        return dict(fused=fused.value, fused_rows=fr.value, loop_rows=lr.value)

    # -- top-k extension (include/glrm_hip_topk.h) -------------------------------------------
    def _topk(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the top-k extension "
                                             "(include/glrm_hip_topk.h is implemented by the HIP engine only)")
        return fn

    @staticmethod
    def _factor_pair(X, Y):
        """Host factors as Fortran-ordered float64 arrays (k x m, k x n), or (None, None) for the handle's resident factors."""
        if (X is None) != (Y is None):
            raise ValueError("X and Y must both be given or both be None (None = the factors resident in the handle)")
        if X is None:
            return None, None
        return np.asfortranarray(X, dtype=np.float64), np.asfortranarray(Y, dtype=np.float64)

    def xy_select(self, h, X, Y, rank):
        """glrm_hip_xy_select: (q, n_gt, n_eq) with q the ``rank``-th largest (1-based) of all u_ij = the ascending fma chain of
        <x_i, y_j> -- ``sort(XY[:], rev=true)[rank]`` -- under Julia's isless (NaN greatest, -0.0 < +0.0), n_gt the entries above q and
        n_eq the entries equal to it.  ``X``, ``Y``: k x m and k x n, or both None for the handle's resident factors."""
        fn = self._topk("xy_select")
        X, Y = self._factor_pair(X, Y)
        q, gt, eq = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        self._ck(fn(h, _ptr(X), _ptr(Y), int(rank), C.byref(q), C.byref(gt), C.byref(eq)))
        return q.value, gt.value, eq.value

    def xy_select_info(self):
        """(passes over X'Y, keys sorted by the early finish) of this thread's last xy_select."""
        fn = self._topk("xy_select_info")
        p, s = C.c_int32(0), C.c_int64(0)
        self._ck(fn(C.byref(p), C.byref(s)))
        return p.value, s.value

    def precision_scan(self, h, X, Y, q, test_rowptr, test_colidx, kprec, block_rows=0, want_hits=True):
        """glrm_hip_precision_scan on the TRAIN model's handle: the loop of src/cross_validate.jl:275-297.  ``test_rowptr`` / ``test_colidx``:
        the test lists as 0-based CSR (m + 1 offsets, column indices).  Returns (true_pos, false_pos, hits, rows_scanned) with hits =
        (rows, cols, is_true) of the entries that counted, in the order of the walk (None without ``want_hits``)."""
        fn = self._topk("precision_scan")
        X, Y = self._factor_pair(X, Y)
        ptr = np.ascontiguousarray(test_rowptr, dtype=np.int64)
        idx = np.ascontiguousarray(test_colidx, dtype=np.int32)
        tp, fp, rows = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        cap = max(int(kprec), 0)
        hr = hc = ht = None
        if want_hits:
            hr, hc, ht = np.full(max(cap, 1), -1, dtype=np.int64), np.full(max(cap, 1), -1, dtype=np.int64), np.zeros(max(cap, 1), dtype=np.uint8)
        self._ck(fn(h, _ptr(X), _ptr(Y), float(q), _ptr(ptr), _ptr(idx) if len(idx) else None, int(kprec), int(block_rows),
                    C.byref(tp), C.byref(fp), _ptr(hr), _ptr(hc), _ptr(ht), C.byref(rows)))
        hits = None
        if want_hits:
            cnt = tp.value + fp.value
            hits = (hr[:cnt].copy(), hc[:cnt].copy(), ht[:cnt].astype(bool))
        return tp.value, fp.value, hits, rows.value

    # -- recommend extension (include/glrm_hip_recommend.h) ----------------------------------
    def _recommend(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the recommend extension "
                                             "(include/glrm_hip_recommend.h is implemented by the HIP engine only)")
        return fn

    def row_topk(self, h, X, Y, rows, kper, exclude=True, col_splits=0, m=None):
        """glrm_hip_row_topk: the ``kper`` best candidates of every query row, best first.  The candidates of a row are all columns, minus
        (``exclude``) the columns in the row's resident (train) list; they are ranked by the key of u_ij descending, then by column
        ascending, under the key of the top-k extension (Julia's isless: NaN greatest, every NaN one value, -0.0 below +0.0), so a NaN
        score ranks first.  ``X``, ``Y``: k x m and k x n, or both None for the handle's resident factors.  ``rows``: 0-based row indices
        in any order, repeats allowed, or None for the rows 0 .. m-1 (m is then read from X, or given as ``m`` with resident factors).
        ``col_splits``: 0 = the engine chooses its column spans, > 0 = that many (the result does not depend on it).  Returns (cols int32 [n_rows, kper], vals float64 [n_rows, kper], count int32 [n_rows]); a row
        with c < kper candidates holds column -1 and the quiet NaN 0x7FF8000000000000 at the positions t >= c, and count = min(kper, c)."""
        fn = self._recommend("row_topk")
        X, Y = self._factor_pair(X, Y)
        if rows is None:
            if X is None and m is None:
                raise ValueError("rows=None (every row) with the resident factors needs m, the number of rows of the handle's problem")
            n_rows, rptr = (X.shape[1] if m is None else int(m)), None
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
            n_rows, rptr = len(rows), _ptr(rows)
        width = max(int(kper), 1)                                    # (kper < 1 is refused by the library; the buffers are never empty)
        cols = np.full((max(n_rows, 1), width), -1, dtype=np.int32)
        vals = np.full((max(n_rows, 1), width), np.nan)
        count = np.zeros(max(n_rows, 1), dtype=np.int32)
        self._ck(fn(h, _ptr(X), _ptr(Y), rptr, n_rows, int(kper), int(exclude), int(col_splits), _ptr(cols), _ptr(vals), _ptr(count)))
        return cols[:n_rows], vals[:n_rows], count[:n_rows]

    def row_topk_info(self) -> dict:
        """Of this thread's last row_topk: ``col_splits`` (the column spans its first block of query rows ran with), ``row_blocks`` and
        ``candidates_merged`` (the entries of the spans' kept lists the final merge read)."""
        fn = self._recommend("row_topk_info")
        s, b, c = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        self._ck(fn(C.byref(s), C.byref(b), C.byref(c)))
        return dict(col_splits=s.value, row_blocks=b.value, candidates_merged=c.value)

    # -- impute_at extension (include/glrm_hip_impute_at.h) ----------------------------------
    def _impute_at(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the impute_at extension "
                                             "(include/glrm_hip_impute_at.h is implemented by the HIP engine only)")
        return fn

    @property
    def has_impute_at(self) -> bool:
        """The library exports the impute_at extension (the CPU oracle does not: a host indexes the full ``impute`` there)."""
        return "impute_at" in self._f

    def impute_at(self, h, X, Y, domains, m, n, rows=None, cols=None, truth=None, block_entries=0, want_err=True, want_total=True):
        """glrm_hip_impute_at: the imputed values of listed entries, and with ``truth`` their errors.  ``rows`` and ``cols`` given (equal
        lengths): the pairs (rows[t], cols[t]), any order, repeats allowed, out of shape (P,).  Only ``rows``: those rows x all ``n``
        columns, out of shape (len(rows), n).  Only ``cols``: all ``m`` rows x those columns, out of shape (m, len(cols)).  Slabs come
        back Fortran-ordered, like ``impute``; every value has the bits the entry has in ``impute``'s matrix.  ``X``, ``Y``: k x m and
        k x d, or both None for the handle's resident factors.  ``domains``: DOMAIN_DTYPE array, one per column.  ``truth``: values of
        out's shape, or None.  ``block_entries``: 0 = the engine chooses how many entries go through the device at a time, > 0 = that
        many (the result does not depend on it).  Returns ``out`` without ``truth``, else ``(out, err, total)`` with err of out's shape
        (None without ``want_err``) and total the sum of err in index order (None without ``want_total``)."""
        fn = self._impute_at("impute_at")
        X, Y = self._factor_pair(X, Y)
        if rows is None and cols is None:
            raise ValueError("impute_at needs rows, cols or both (every entry of the model is `impute`)")
        m, n = int(m), int(n)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if cols is not None:
            cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        if rows is not None and cols is not None:
            mode, shape = IMPUTE_AT_PAIRS, (len(rows),)
            if len(rows) != len(cols):
                raise ValueError(f"pairs need as many rows as cols, got {len(rows)} and {len(cols)}")
        elif rows is not None:
            mode, shape = IMPUTE_AT_ROWS, (len(rows), n)
        else:
            mode, shape = IMPUTE_AT_COLS, (m, len(cols))
        total = int(np.prod(shape))
        if truth is not None:
            truth = np.asfortranarray(truth, dtype=np.float64)
            if truth.shape != shape:
                raise ValueError(f"truth has shape {truth.shape}, the queried entries {shape}")
        flat = max(total, 1)                                         # (the buffers are never empty)
        out = np.full(flat, np.nan)
        err = np.full(flat, np.nan) if truth is not None and want_err else None
        tot = C.c_double(np.nan)
        tbuf = None if truth is None else truth if total else np.zeros(1)
        self._ck(fn(h, _ptr(X), _ptr(Y), _ptr(domains), _ptr(rows) if rows is not None and len(rows) else None, 0 if rows is None else len(rows),
                    _ptr(cols) if cols is not None and len(cols) else None, 0 if cols is None else len(cols), mode,
                    _ptr(tbuf), int(block_entries), _ptr(out), _ptr(err), C.byref(tot) if truth is not None and want_total else None))
        out = out[:total].reshape(shape, order="F")
        if truth is None:
            return out
        return out, (err[:total].reshape(shape, order="F") if err is not None else None), (tot.value if want_total else None)

    def impute_at_info(self) -> dict:
        """Of this thread's last impute_at: ``blocks`` (the blocks the entries went through the device in), ``entries_fast`` (scalar-loss
        entries: the coalesced gather kernel) and ``entries_general`` (entries of multi-dimensional columns)."""
        fn = self._impute_at("impute_at_info")
        b, f, g = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ck(fn(C.byref(b), C.byref(f), C.byref(g)))
        return dict(blocks=b.value, entries_fast=f.value, entries_general=g.value)


    # -- sampling extension (include/glrm_hip_sample.h) ----------------------------------------
    def _sample(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the sampling extension "
                                             "(include/glrm_hip_sample.h is implemented by the HIP engine only)")
        return fn

    def sample_at(self, h, X, Y, domains, m, n, rows=None, cols=None, *, seed, noise="residual", noise_sd=None, keep_observed=False,
                  block_entries=0, want_kept=True, want_noise_sd=True):
        """glrm_hip_sample_at: a draw from the model at every listed entry; ``rows`` / ``cols`` / the shape of the result as for
        ``impute_at``.  ``seed``: the 64-bit key of the generator -- a draw is a function of (seed, row, column, X, Y, lists) alone.
        ``noise``: "residual" (sd_j = sqrt(v_j)), "reference" (1 / sqrt(v_j)) or "given" (``noise_sd``, n values).  ``keep_observed``:
        an entry whose column is in its row's resident row-view list returns the stored value.  Returns ``(out, kept, noise_sd)``:
        ``kept`` (bool, out's shape) with ``keep_observed`` and ``want_kept``, else None; ``noise_sd`` (n values, NaN outside the
        Real x QuadLoss columns) with ``want_noise_sd``, else None."""
        fn = self._sample("sample_at")
        X, Y = self._factor_pair(X, Y)
        if rows is None and cols is None:
            raise ValueError("sample_at needs rows, cols or both (every entry of the model is `sample`)")
        m, n = int(m), int(n)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if cols is not None:
            cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        if rows is not None and cols is not None:
            mode, shape = IMPUTE_AT_PAIRS, (len(rows),)
            if len(rows) != len(cols):
                raise ValueError(f"pairs need as many rows as cols, got {len(rows)} and {len(cols)}")
        elif rows is not None:
            mode, shape = IMPUTE_AT_ROWS, (len(rows), n)
        else:
            mode, shape = IMPUTE_AT_COLS, (m, len(cols))
        total = int(np.prod(shape))
        if noise not in SAMPLE_NOISE:
            raise ValueError(f"noise must be one of {sorted(SAMPLE_NOISE)}, got {noise!r}")
        if noise_sd is not None:
            noise_sd = np.ascontiguousarray(noise_sd, dtype=np.float64).reshape(-1)
            if len(noise_sd) != n:
                raise ValueError(f"noise_sd has {len(noise_sd)} values for {n} columns")
        flat = max(total, 1)                                         # (the buffers are never empty)
        out = np.full(flat, np.nan)
        kept = np.zeros(flat, dtype=np.uint8) if keep_observed and want_kept else None
        sd = np.full(max(n, 1), np.nan) if want_noise_sd else None
        self._ck(fn(h, _ptr(X), _ptr(Y), _ptr(domains), _ptr(rows) if rows is not None and len(rows) else None, 0 if rows is None else len(rows),
                    _ptr(cols) if cols is not None and len(cols) else None, 0 if cols is None else len(cols), mode,
                    int(seed) & 0xFFFFFFFFFFFFFFFF, SAMPLE_NOISE[noise], _ptr(noise_sd), int(bool(keep_observed)), int(block_entries),
                    _ptr(out), _ptr(kept), _ptr(sd)))
        return (out[:total].reshape(shape, order="F"), None if kept is None else kept[:total].astype(bool).reshape(shape, order="F"),
                None if sd is None else sd[:n])

    def sample_at_info(self) -> dict:
        """Of this thread's last sample_at: ``blocks``, ``entries_fast``, ``entries_general`` (as for impute_at), ``entries_kept``
        (entries that kept their observed value) and ``variance_columns`` (columns the variance pass computed; 0: it did not run)."""
        fn = self._sample("sample_at_info")
        v = [C.c_int64(0) for _ in range(5)]
        self._ck(fn(*[C.byref(x) for x in v]))
        return dict(zip(("blocks", "entries_fast", "entries_general", "entries_kept", "variance_columns"), (x.value for x in v)))

    # -- ALS extension (include/glrm_hip_als.h) ----------------------------------------------
    def _als(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the ALS extension "
                                             "(include/glrm_hip_als.h is implemented by the HIP engine only)")
        return fn

    @property
    def has_als(self) -> bool:
        """The library exports the ALS extension (the CPU oracle does not)."""
        return "als_solve" in self._f

    def als_solve(self, h, side):
        """glrm_hip_als_solve: every local row of X (``side`` 0) or column of Y (1) replaced by the exact minimiser of its part of the
        objective with the opposing factor as it stands (QuadLoss columns, QuadReg / ZeroReg on the solved side).  Asynchronous."""
        self._ck(self._als("als_solve")(h, int(side)))

    def als_info(self, h, side, nseg=None) -> dict:
        """What the last als_solve of ``side`` did: ``solved``, ``kept_short`` (penalty scale 0 and fewer than k observations) and
        ``kept_pivot`` (a pivot failed the rank rule) segments; with ``nseg`` (the local segments of the side) also ``status``, one int8
        per segment (ALS_SOLVED / ALS_KEPT_SHORT / ALS_KEPT_PIVOT).  Synchronises."""
        fn = self._als("als_info")
        n = [C.c_int64(0) for _ in range(3)]
        status = None if nseg is None else np.full(max(int(nseg), 1), -1, dtype=np.int8)
        self._ck(fn(h, int(side), C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), _ptr(status)))
        out = dict(solved=n[0].value, kept_short=n[1].value, kept_pivot=n[2].value)
        if status is not None:
            out["status"] = status[: int(nseg)]
        return out

    # -- coordinate-descent extension (include/glrm_hip_cd.h) ---------------------------------
    def _cd(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the coordinate-descent extension "
                                             "(include/glrm_hip_cd.h is implemented by the HIP engine only)")
        return fn

    @property
    def has_cd(self) -> bool:
        """The library exports the coordinate-descent extension (the CPU oracle does not)."""
        return "cd_solve" in self._f

    def cd_solve(self, h, side, sweeps):
        """glrm_hip_cd_solve: at most ``sweeps`` cyclic coordinate-descent sweeps on every local row of X (``side`` 0) or column of Y (1)
        with the opposing factor as it stands (QuadLoss columns; ZeroReg, QuadReg, OneReg or NonNegConstraint on the solved side).
        Asynchronous."""
        self._ck(self._cd("cd_solve")(h, int(side), int(sweeps)))

    def cd_info(self, h, side, nseg=None) -> dict:
        """What the last cd_solve of ``side`` did: the segments that stopped because a whole sweep changed no bit (``converged``), those
        with a coordinate that failed the denominator rule (``skipped``) and the sweeps run summed over the segments (``sweeps_total``);
        with ``nseg`` (the local segments of the side) also ``status`` (int8 bits CD_CONVERGED / CD_SKIPPED) and ``sweeps_run`` (int32)
        per segment.  Synchronises."""
        fn = self._cd("cd_info")
        n = [C.c_int64(0) for _ in range(3)]
        status = None if nseg is None else np.full(max(int(nseg), 1), -1, dtype=np.int8)
        run = None if nseg is None else np.full(max(int(nseg), 1), -1, dtype=np.int32)
        self._ck(fn(h, int(side), C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), _ptr(status), _ptr(run)))
        out = dict(converged=n[0].value, skipped=n[1].value, sweeps_total=n[2].value)
        if status is not None:
            out["status"], out["sweeps_run"] = status[: int(nseg)], run[: int(nseg)]
        return out

    # -- streaming extension (include/glrm_hip_stream.h) ---------------------------------------
    def _stream(self, name):
        fn = self._f.get(name)
        if fn is None:
            raise GLRMError(ERR_UNSUPPORTED, f"{self.prefix}{name}: this engine does not have the streaming extension "
                                             "(include/glrm_hip_stream.h is implemented by the HIP engine only)")
        return fn

    @property
    def has_stream(self) -> bool:
        """The library exports the streaming extension (the CPU oracle does not)."""
        return "stream_rows" in self._f

    @staticmethod
    def _queries(qptr, qcol):
        if (qptr is None) != (qcol is None):
            raise GLRMError(ERR_INVALID, "qptr and qcol go together (both, or neither)")
        if qptr is None:
            return None, None
        return np.ascontiguousarray(qptr, dtype=np.int64), np.ascontiguousarray(qcol, dtype=np.int32)

    def stream_plan(self, m, n, first, rowptr, colidx, qptr=None, qcol=None, sequential=False) -> dict:
        """glrm_hip_stream_plan (pure host code): the level of every row first .. m-1 of a CSR row view and the plan's figures ->
        dict(level, nlevels, nlaunches, max_width, dup_rows)."""
        fn = self._stream("stream_plan")
        rowptr, colidx = np.ascontiguousarray(rowptr, dtype=np.int64), np.ascontiguousarray(colidx, dtype=np.int32)
        if len(rowptr) != int(m) + 1 or len(colidx) < int(rowptr[-1]):
            raise GLRMError(ERR_INVALID, "stream_plan: rowptr holds m + 1 offsets and colidx rowptr[m] columns")
        qptr, qcol = self._queries(qptr, qcol)
        if qptr is not None and (len(qptr) != int(m) + 1 or len(qcol) < int(qptr[-1])):
            raise GLRMError(ERR_INVALID, "stream_plan: qptr holds m + 1 offsets and qcol qptr[m] columns")
        level = np.zeros(max(int(m) - int(first), 1), dtype=np.int64)
        v = [C.c_int64(0) for _ in range(4)]
        self._ck(fn(int(m), int(n), int(first), _ptr(rowptr), _ptr(colidx), _ptr(qptr), _ptr(qcol), 1 if sequential else 0, _ptr(level),
                    *[C.byref(x) for x in v]))
        return dict(level=level[: max(int(m) - int(first), 0)], nlevels=v[0].value, nlaunches=v[1].value, max_width=v[2].value, dup_rows=v[3].value)

    def stream_rows(self, h, m, first, stepsize, interval, sequential=False, qptr=None, qcol=None, want_objective=True):
        """glrm_hip_stream_rows: rows ``first`` .. m-1 of the handle streamed once over the resident X and Y (``m``: the handle's rows).
        ``qptr`` / ``qcol``: the queries of every row (m + 1 offsets, columns).  Synchronises -> (objective per streamed row or None,
        query results or None)."""
        fn = self._stream("stream_rows")
        qptr, qcol = self._queries(qptr, qcol)
        if qptr is not None and (len(qptr) != int(m) + 1 or len(qcol) < int(qptr[-1])):
            raise GLRMError(ERR_INVALID, "stream_rows: qptr holds m + 1 offsets and qcol qptr[m] columns")
        rows = max(int(m) - int(first), 0)
        obj = np.full(max(rows, 1), np.nan) if want_objective else None
        qout = None if qptr is None else np.full(max(int(qptr[-1]), 1), np.nan)
        self._ck(fn(h, int(first), float(stepsize), int(interval), 1 if sequential else 0, _ptr(qptr), _ptr(qcol), _ptr(qout), _ptr(obj)))
        return (None if obj is None else obj[:rows]), (None if qout is None else qout[: int(qptr[-1])])

    def stream_info(self, h, rows=None) -> dict:
        """What the last stream_rows did: ``solved`` / ``kept_short`` / ``kept_pivot`` rows, the plan's ``nlevels`` / ``nlaunches`` /
        ``max_width`` and ``plan_ms``; with ``rows`` (the rows streamed) also ``status``, one int8 per streamed row (ALS_*)."""
        fn = self._stream("stream_info")
        v = [C.c_int64(0) for _ in range(6)]
        ms = C.c_double(0.0)
        status = None if rows is None else np.full(max(int(rows), 1), -1, dtype=np.int8)
        self._ck(fn(h, *[C.byref(x) for x in v], C.byref(ms), _ptr(status)))
        out = dict(zip(("solved", "kept_short", "kept_pivot", "nlevels", "nlaunches", "max_width"), (x.value for x in v)))
        out["plan_ms"] = ms.value
        if status is not None:
            out["status"] = status[: int(rows)]
        return out


class ProblemArrays:
    """Plain container for one shard in the ABI's layout (0-based, CSR + CSC, descriptors)."""

    def __init__(self, m, n, k, rowptr, colidx, rowvals, colptr, rowidx, colvals, losses, rx, ry,
                 row_begin=0, row_end=None, col_begin=0, col_end=None, flags=0, dense_A=None, dense_ld=0, dense_colmajor=0):
        self.m, self.n, self.k, self.flags = int(m), int(n), int(k), int(flags)
        self.row_begin, self.row_end = int(row_begin), int(m if row_end is None else row_end)
        self.col_begin, self.col_end = int(col_begin), int(n if col_end is None else col_end)
        self.rowptr, self.colidx, self.rowvals = rowptr, colidx, rowvals
        self.colptr, self.rowidx, self.colvals = colptr, rowidx, colvals
        self.losses, self.rx, self.ry = losses, rx, ry  # numpy structured arrays (LOSS_DTYPE / REG_DTYPE)
        # fully observed QuadLoss hand-over: the whole m x n matrix (numpy array or device address) instead of lists
        self.dense_A, self.dense_ld, self.dense_colmajor = dense_A, int(dense_ld), int(dense_colmajor)

    @property
    def ystart(self):
        """Column f owns vectors [ystart[f], ystart[f+1]) of Y (get_yidxs, src/losses.jl:76-93)."""
        dims = np.maximum(np.asarray(self.losses["dim"], dtype=np.int64), 1)
        if len(dims) == 1:
            return np.arange(self.n + 1, dtype=np.int64) * int(dims[0])
        return np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)

    @property
    def d(self):
        """Vectors of Y = sum of the embedding dimensions (= n for scalar losses)."""
        return int(self.ystart[-1])


_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# GLRM_HIP_LIB_PATH: another BUILD of the same engine (tests/perf/ab_lib.py, variant builds of build.py) -- never another engine
HIP_LIB_PATH = os.environ.get("GLRM_HIP_LIB_PATH") or os.path.join(_PKG_DIR, "libglrm_hip.so")
_hip_api = None


HIP_TESTING_LIB_PATH = os.path.join(_PKG_DIR, "libglrm_hip_testing.so")
_hip_testing_api = None


def hip_testing_api() -> Api:
    """The TEST BUILD of the engine (libglrm_hip_testing.so: the product objects with csrc/glrm_testhooks.hip and csrc/glrm_multigpu.hip rebuilt
    under -DGLRM_HIP_TESTING): the only library in which GLRM_HIP_TEST_FAIL_FINALIZE, GLRM_HIP_RCCL_LIB / GLRM_HIP_RCCL_ALLOW_SHARED and the
    link emulator (GLRM_EXCHANGE_EMULATE_*) exist.  For tests and `bench.py --emulate-link-gbps`; never what `fit_b` runs on."""
    global _hip_testing_api
    if _hip_testing_api is None:
        if not os.path.exists(HIP_TESTING_LIB_PATH):
            raise RuntimeError(f"{HIP_TESTING_LIB_PATH} is missing: build it with `python __graft_entry__.py`")
        _hip_testing_api = Api(C.CDLL(HIP_TESTING_LIB_PATH, mode=C.RTLD_LOCAL), "glrm_hip_", "cuda")
    return _hip_testing_api


def hip_api() -> Api:
    """The MI355X engine.  Fails loudly when the HIP library has not been built -- there is no
    CPU fallback in the product path."""
    global _hip_api
    if _hip_api is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise RuntimeError(
                f"{HIP_LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
                "lowrankmodels.jl_amd has no CPU fallback."
            )
        _hip_api = Api(C.CDLL(HIP_LIB_PATH, mode=C.RTLD_GLOBAL), "glrm_hip_", "cuda")
    return _hip_api
