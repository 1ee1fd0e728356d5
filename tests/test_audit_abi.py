"""CPU: the entry points of the constraint audit and of the single-edge edits (kh_spa_audit_constraints, kh_mapper_add_edge,
kh_mapper_remove_edge, kh_mapper_correct_poses, kh_mapper_audit, kh_reject_params_default, kh_mapper_reject_outliers) are exported
and bound with prototypes, the structs have the header's layout, the defaults are the documented ones, and every invalid argument
is refused with KH_ERR_INVALID_ARG before a device is looked for.  (No solver or mapper can exist without a device, so the handle
is NULL throughout.)"""
import ctypes as C
import os
import re

import numpy as np

from slam_toolbox_amd import capi

NEW = ("kh_spa_audit_constraints", "kh_mapper_add_edge", "kh_mapper_remove_edge", "kh_mapper_correct_poses", "kh_mapper_audit",
       "kh_mapper_reject_outliers")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "karto_hip.h")


def without_a_device(lib, rc):
    if lib.kh_device_count() > 0:
        assert rc == capi.KH_ERR_INVALID_ARG                   # a device is visible: the NULL handle is what is wrong
    else:
        assert rc == capi.KH_ERR_NO_DEVICE and b"no CPU fallback" in lib.kh_last_error()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_new_entry_points_are_exported_and_bound(kartohip_lib):
    text = open(HEADER).read()
    for name in NEW:
        assert hasattr(kartohip_lib, name), name
        assert name in capi.SYMBOLS and getattr(kartohip_lib, name).argtypes is not None, name
        assert re.search(r"KH_API int " + name + r"\(", text), name
    assert hasattr(kartohip_lib, "kh_reject_params_default") and "kh_reject_params_default" in capi.SYMBOLS
    assert re.search(r"KH_API void kh_reject_params_default\(", text)


def test_structs_match_the_header():
    A, S, P, R = capi.KhSpaAudit, capi.KhSpaAuditSummary, capi.KhRejectParams, capi.KhRejectSummary
    assert C.sizeof(A) == 4 * 4 + 4 * 8 == capi.AUDIT_DTYPE.itemsize
    assert [k for k, _ in A._fields_] == list(capi.AUDIT_DTYPE.names) == ["index", "id_a", "id_b", "verifiable", "chi2", "redundancy",
                                                                          "min_pivot", "chi2_loo"]
    assert [capi.AUDIT_DTYPE.fields[k][1] for k in capi.AUDIT_DTYPE.names] == [getattr(A, k).offset for k in capi.AUDIT_DTYPE.names]
    assert C.sizeof(S) == C.sizeof(capi.KhSpaCovSummary) + 2 * 4 + 2 * 8 and S.n_constraints.offset == C.sizeof(capi.KhSpaCovSummary)
    assert C.sizeof(P) == 3 * 8 + 2 * 4 and P.min_id_gap.offset == 24 and P.max_rounds.offset == 28
    assert C.sizeof(R) == 2 * 4 + 4 * 8 and R.max_chi2_loo.offset == 8
    text = open(HEADER).read()
    body = re.search(r"typedef struct kh_spa_audit_t \{(.*?)\} kh_spa_audit_t;", text, re.S).group(1)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == [k for k, _ in A._fields_]
    body = re.search(r"typedef struct kh_reject_params \{(.*?)\} kh_reject_params;", text, re.S).group(1)
    assert re.findall(r"(?:int32_t|double) (\w+);", body) == [k for k, _ in P._fields_]
    body = re.search(r"typedef struct kh_reject_summary \{(.*?)\} kh_reject_summary;", text, re.S).group(1)
    assert [w for decl in re.findall(r"(?:int32_t|double) ([\w, ]+);", body) for w in decl.replace(" ", "").split(",")] == [k for k, _ in R._fields_]
    # the structs that were there are as they were
    assert C.sizeof(capi.KhMapperStats) == 18 * 8 and C.sizeof(capi.KhSpaCovSummary) == 4 * 4 + 6 * 8


def test_defaults(kartohip_lib):
    p = capi.KhRejectParams()
    kartohip_lib.kh_reject_params_default(C.byref(p))
    assert (p.chi2, p.min_redundancy, p.tie, p.min_id_gap, p.max_rounds) == (16.266, 1e-6, 1e-6, 2, 8)
    kartohip_lib.kh_reject_params_default(None)                            # (nothing to write to: no effect)
    import inspect
    from slam_toolbox_amd.mapper import Mapper
    from slam_toolbox_amd.scan_solver import HipSpaSolver
    assert inspect.signature(HipSpaSolver.AuditConstraints).parameters["min_redundancy"].default == 1e-6
    assert inspect.signature(Mapper.audit).parameters["min_redundancy"].default == 1e-6
    for name in ("AddEdge", "RemoveEdge", "CorrectPoses", "audit", "RejectOutliers"):
        assert callable(getattr(Mapper, name))


def test_bad_arguments_are_refused_before_a_device_is_looked_for(kartohip_lib):
    L = kartohip_lib
    out = np.zeros(8, dtype=capi.AUDIT_DTYPE)
    s = capi.KhSpaAuditSummary()
    for bad in (0.0, 1.0, -1e-6, 2.0, float("nan"), float("inf"), -float("inf")):
        assert L.kh_spa_audit_constraints(None, bad, ptr(out), C.byref(s)) == capi.KH_ERR_INVALID_ARG, bad
        n = C.c_int32(-1)
        assert L.kh_mapper_audit(None, bad, ptr(out), 8, C.byref(n), C.byref(s)) == capi.KH_ERR_INVALID_ARG, bad
    assert L.kh_spa_audit_constraints(None, 1e-6, None, C.byref(s)) == capi.KH_ERR_INVALID_ARG
    n = C.c_int32(-1)
    assert L.kh_mapper_audit(None, 1e-6, None, 8, C.byref(n), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_audit(None, 1e-6, ptr(out), 8, None, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_audit(None, 1e-6, ptr(out), -1, C.byref(n), None) == capi.KH_ERR_INVALID_ARG
    mean, cov = np.zeros(3), np.eye(3).reshape(9)
    assert L.kh_mapper_add_edge(None, 0, 1, None, ptr(cov), 0) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_add_edge(None, 0, 1, ptr(mean), None, 0) == capi.KH_ERR_INVALID_ARG
    bad_mean = np.array([0.0, float("nan"), 0.0])
    assert L.kh_mapper_add_edge(None, 0, 1, ptr(bad_mean), ptr(cov), 1) == capi.KH_ERR_INVALID_ARG
    good = capi.KhRejectParams()
    L.kh_reject_params_default(C.byref(good))
    sm = capi.KhRejectSummary()
    for field, value in (("min_id_gap", 0), ("min_id_gap", -2), ("max_rounds", 0), ("max_rounds", -1), ("tie", -1e-9), ("tie", 1.0),
                         ("tie", float("nan")), ("tie", float("inf")), ("chi2", float("nan")), ("chi2", float("inf")), ("chi2", -1.0),
                         ("min_redundancy", 0.0), ("min_redundancy", 1.0), ("min_redundancy", float("nan")),
                         ("min_redundancy", float("inf"))):
        p = capi.KhRejectParams.from_buffer_copy(good)
        setattr(p, field, value)
        assert L.kh_mapper_reject_outliers(None, C.byref(p), ptr(out), 8, C.byref(sm)) == capi.KH_ERR_INVALID_ARG, (field, value)
    assert L.kh_mapper_reject_outliers(None, C.byref(good), None, 8, None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_reject_outliers(None, C.byref(good), ptr(out), -1, None) == capi.KH_ERR_INVALID_ARG


def test_valid_calls_without_a_device_are_no_device(kartohip_lib):
    L = kartohip_lib
    out = np.zeros(8, dtype=capi.AUDIT_DTYPE)
    s = capi.KhSpaAuditSummary()
    n = C.c_int32(0)
    mean, cov = np.zeros(3), np.eye(3).reshape(9)
    good = capi.KhRejectParams()
    L.kh_reject_params_default(C.byref(good))
    for md in (1e-6, 1e-12, 0.5):
        without_a_device(L, L.kh_spa_audit_constraints(None, md, ptr(out), C.byref(s)))
    without_a_device(L, L.kh_spa_audit_constraints(None, 1e-6, ptr(out), None))
    without_a_device(L, L.kh_mapper_audit(None, 1e-6, ptr(out), 8, C.byref(n), C.byref(s)))
    without_a_device(L, L.kh_mapper_add_edge(None, 2, 55, ptr(mean), ptr(cov), 1))
    without_a_device(L, L.kh_mapper_remove_edge(None, 2, 55))
    without_a_device(L, L.kh_mapper_correct_poses(None))
    without_a_device(L, L.kh_mapper_reject_outliers(None, C.byref(good), ptr(out), 8, None))
    without_a_device(L, L.kh_mapper_reject_outliers(None, None, None, 0, None))          # (no parameters: the defaults)
    good.tie = 0.0
    without_a_device(L, L.kh_mapper_reject_outliers(None, C.byref(good), ptr(out), 8, None))
