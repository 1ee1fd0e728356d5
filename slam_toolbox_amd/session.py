"""Mapping session files (kh_mapper_save / kh_mapper_load): `info(path)` asks the library (kh_session_info: header and full
structural check, no device needed); `read(path)` is a numpy reader of the same format written from the description in DESIGN.md
section 7, not from the C code -- the tests hold the two against each other.

    "KHMS"  u32 version  u64 file size  u32 sections  u32 crc32 (zlib's, of every byte behind these 24)
    per section: 4-byte tag, u32 0, u64 offset, u64 size          (11 entries; the sections follow in this order)
    PARM LASR LIFE STAT RUNB SCAN RNGS ADJL SNOD SCON SANA         little endian, every section a multiple of 8 bytes
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib

import numpy as np

from . import capi

MAGIC, VERSION = b"KHMS", 1
TAGS = ("PARM", "LASR", "LIFE", "STAT", "RUNB", "SCAN", "RNGS", "ADJL", "SNOD", "SCON", "SANA")
HEADER_BYTES, ENTRY_BYTES = 24, 24
# kh_mapper_params in declaration order: "i" = int32 stored as int64, "d" = double
PARAM_WORDS = (("use_scan_matching", "i"), ("use_scan_barycenter", "i"), ("minimum_time_interval", "d"), ("minimum_travel_distance", "d"),
               ("minimum_travel_heading", "d"), ("scan_buffer_size", "i"), ("scan_buffer_maximum_scan_distance", "d"),
               ("link_match_minimum_response_fine", "d"), ("link_scan_maximum_distance", "d"), ("loop_search_maximum_distance", "d"),
               ("do_loop_closing", "i"), ("loop_match_minimum_chain_size", "i"), ("loop_match_maximum_variance_coarse", "d"),
               ("loop_match_minimum_response_coarse", "d"), ("loop_match_minimum_response_fine", "d"),
               ("correlation_search_space_dimension", "d"), ("correlation_search_space_resolution", "d"),
               ("correlation_search_space_smear_deviation", "d"), ("loop_search_space_dimension", "d"), ("loop_search_space_resolution", "d"),
               ("loop_search_space_smear_deviation", "d"), ("coarse_search_angle_offset", "d"), ("coarse_angle_resolution", "d"),
               ("fine_search_angle_offset", "d"), ("use_response_expansion", "i"), ("distance_variance_penalty", "d"),
               ("minimum_distance_penalty", "d"), ("angle_variance_penalty", "d"), ("minimum_angle_penalty", "d"))
LASER_WORDS = ("n_beams", "minimum_angle", "angular_resolution", "minimum_range", "maximum_range", "range_threshold", "offset_x", "offset_y",
               "offset_heading")
DECAY_WORDS = ("iou_thresh", "iou_match", "removal_score", "overlap_scale", "constraint_scale", "nearby_penalty", "candidates_scale")


class SessionFormatError(ValueError):
    pass


def info(path) -> dict:
    """kh_session_info: the counts of a session file after the library's full structural check (KartoHipError, status
    KH_ERR_IO, for a file it rejects)"""
    out = capi.KhSessionInfo()
    capi.check(capi.lib().kh_session_info(str(path).encode(), C.byref(out)), "kh_session_info")
    return {k: int(getattr(out, k)) for k, _ in capi.KhSessionInfo._fields_}


def sections(data: bytes):
    """[(tag, offset, size)] of the section table, after the header checks"""
    if len(data) < HEADER_BYTES:
        raise SessionFormatError("truncated inside the header")
    magic, version, size, n_sections, crc = struct.unpack_from("<4sIQII", data, 0)
    if magic != MAGIC:
        raise SessionFormatError("wrong magic")
    if version != VERSION:
        raise SessionFormatError(f"unknown version {version}")
    if size != len(data):
        raise SessionFormatError("truncated")
    if n_sections != len(TAGS) or len(data) < HEADER_BYTES + ENTRY_BYTES * n_sections:
        raise SessionFormatError("section table does not fit")
    if zlib.crc32(data[HEADER_BYTES:]) & 0xFFFFFFFF != crc:
        raise SessionFormatError("checksum mismatch")
    out, at = [], HEADER_BYTES + ENTRY_BYTES * n_sections
    for k, want in enumerate(TAGS):
        tag, zero, off, size_k = struct.unpack_from("<4sIQQ", data, HEADER_BYTES + ENTRY_BYTES * k)
        if tag.decode("ascii", "replace") != want or zero != 0 or off != at or size_k % 8 or off + size_k > len(data):
            raise SessionFormatError(f"section {want} does not fit the file")
        out.append((want, off, size_k))
        at += size_k
    if at != len(data):
        raise SessionFormatError("bytes behind the last section")
    return out


def read(path) -> dict:
    """The whole state of a session file as numpy arrays and plain dicts."""
    with open(path, "rb") as f:
        data = f.read()
    sec = {tag: data[off:off + size] for tag, off, size in sections(data)}

    def take(buf, at, dtype, count):
        n = np.dtype(dtype).itemsize * count
        if at + n > len(buf):
            raise SessionFormatError("counts do not fit the section")
        return np.frombuffer(buf, dtype=dtype, count=count, offset=at).copy(), at + n

    def pad8(at):
        return (at + 7) & ~7

    out = {}
    words, _ = take(sec["PARM"], 0, "<u8", len(PARAM_WORDS))
    out["params"] = {name: (int(w.astype(np.int64)) if kind == "i" else float(w.view(np.float64))) for (name, kind), w in zip(PARAM_WORDS, words)}
    words, _ = take(sec["LASR"], 0, "<u8", len(LASER_WORDS))
    out["laser"] = {name: (int(w.astype(np.int64)) if name == "n_beams" else float(w.view(np.float64))) for name, w in zip(LASER_WORDS, words)}
    words, _ = take(sec["LIFE"], 0, "<u8", 9)
    out["lifelong"] = int(words[0])
    out["decay"] = {name: float(w.view(np.float64)) for name, w in zip(DECAY_WORDS, words[1:8])}
    out["decay"]["scan_buffer_size"] = int(words[8].astype(np.int64))
    stat, _ = take(sec["STAT"], 0, "<i8", 6)
    n_slots, n_alive, n_edges, last, n_running, n_loc = (int(v) for v in stat)
    out.update(n_scan_slots=n_slots, n_alive=n_alive, n_edges=n_edges, last_scan=last)
    out["running"], at = take(sec["RUNB"], 0, "<i4", n_running)
    out["localization_buffer"], at = take(sec["RUNB"], at, "<i4", n_loc)
    if pad8(at) != len(sec["RUNB"]):
        raise SessionFormatError("counts do not fit section RUNB")
    n_beams = out["laser"]["n_beams"]
    rec = np.dtype([("id", "<i4"), ("zero", "<i4"), ("time", "<f8"), ("odometric", "<f8", 3), ("corrected", "<f8", 3), ("score", "<f8")])
    assert rec.itemsize == 72
    if len(sec["SCAN"]) != 72 * n_alive or len(sec["RNGS"]) != 8 * n_alive * n_beams:
        raise SessionFormatError("counts do not fit sections SCAN / RNGS")
    scans = np.frombuffer(sec["SCAN"], dtype=rec, count=n_alive)
    out["ids"] = scans["id"].copy()
    out["time"], out["odometric"], out["corrected"], out["score"] = (scans[k].copy() for k in ("time", "odometric", "corrected", "score"))
    out["ranges"] = np.frombuffer(sec["RNGS"], dtype="<f8", count=n_alive * n_beams).reshape(n_alive, n_beams).copy()
    adj_count, at = take(sec["ADJL"], 0, "<i4", n_slots)
    out_count, at = take(sec["ADJL"], at, "<i4", n_slots)
    adj, at = take(sec["ADJL"], at, "<i4", int(adj_count.sum()))
    outs, at = take(sec["ADJL"], at, "<i4", int(out_count.sum()))
    if pad8(at) != len(sec["ADJL"]):
        raise SessionFormatError("counts do not fit section ADJL")
    out["adj_count"], out["out_count"], out["adj"], out["out_edges"] = adj_count, out_count, adj, outs
    head, at = take(sec["SNOD"], 0, "<i8", 8)
    n_nodes = int(head[0])
    out["solver_gauge"] = {"has_first": int(head[1]), "first_id": int(head[2]), "was_constant_set": int(head[3])}
    out["solver_analysis"] = {"full_flops": int(head[4]), "full_free_nodes": int(head[5]), "reuse_count": int(head[6]), "full_levels": int(head[7])}
    out["node_ids"], at = take(sec["SNOD"], at, "<i4", n_nodes)
    out["node_poses"], at = take(sec["SNOD"], pad8(at), "<f8", 3 * n_nodes)
    out["node_poses"] = out["node_poses"].reshape(n_nodes, 3)
    if at != len(sec["SNOD"]):
        raise SessionFormatError("counts do not fit section SNOD")
    head, at = take(sec["SCON"], 0, "<i8", 1)
    m = int(head[0])
    out["constraint_a"], at = take(sec["SCON"], at, "<i4", m)
    out["constraint_b"], at = take(sec["SCON"], at, "<i4", m)
    z, at = take(sec["SCON"], at, "<f8", 3 * m)
    inf, at = take(sec["SCON"], at, "<f8", 6 * m)
    out["constraint_z"], out["constraint_information"] = z.reshape(m, 3), inf.reshape(m, 6)
    if at != len(sec["SCON"]):
        raise SessionFormatError("counts do not fit section SCON")
    head, at = take(sec["SANA"], 0, "<i8", 1)
    out["supernode_ptr"], at = take(sec["SANA"], at, "<i4", int(head[0]) + 1)
    out["supernode_ids"], at = take(sec["SANA"], at, "<i4", int(out["supernode_ptr"][-1]))
    if pad8(at) != len(sec["SANA"]):
        raise SessionFormatError("counts do not fit section SANA")
    return out
