"""CPU: the mapping-session file format (kh_mapper_save / kh_mapper_load / kh_session_info, slam_toolbox_amd/session.py).

tests/golden/session_small.khms was written by kh_mapper_save on the GPU (tests/golden/make_golden_session.py: 181-beam laser,
the lap queue up to six scans behind its first loop closure, node 20 removed, four scans in the localization buffer);
session_small.npz holds the same state dumped through the getters at save time.  Here, without a device: the library's structural
check accepts the file and reports its counts, the independent numpy reader returns every array bit for bit, and every damaged
variant of the file is refused with KH_ERR_IO and a text -- never a crash or an over-read."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from common import bits
from slam_toolbox_amd import capi, session

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KHMS, NPZ = os.path.join(GOLDEN, "session_small.khms"), os.path.join(GOLDEN, "session_small.npz")


@pytest.fixture(scope="module")
def good():
    with open(KHMS, "rb") as f:
        return f.read()


def _info_status(path):
    out = capi.KhSessionInfo()
    return capi.lib().kh_session_info(str(path).encode(), C.byref(out)), capi.lib().kh_last_error().decode()


def _load_status(path):
    h = C.c_void_p()
    rc = capi.lib().kh_mapper_load(str(path).encode(), np.zeros(1, dtype=np.int32), 1, 32, C.byref(h))
    if rc == capi.KH_OK:
        capi.lib().kh_mapper_destroy(h)
    return rc, capi.lib().kh_last_error().decode()


def _with_checksum(data: bytes) -> bytes:
    """the file with its checksum recomputed (a damaged count must be caught by the size check, not by the CRC)"""
    return data[:20] + struct.pack("<I", zlib.crc32(data[24:]) & 0xFFFFFFFF) + data[24:]


def test_info_reports_the_counts(kartohip_lib, good):
    ref = np.load(NPZ)
    info = session.info(KHMS)
    assert info["version"] == 1 and info["file_bytes"] == len(good) and info["n_beams"] == int(ref["n_beams"]) == 181
    assert info["n_scan_slots"] == int(ref["n_scan_slots"]) and info["n_alive"] == len(ref["alive"]) == info["n_scan_slots"] - 1
    assert info["n_edges"] == int(ref["n_edges"]) and info["n_localization_buffer"] == len(ref["localization_buffer"]) == 4
    assert info["n_solver_nodes"] == len(ref["node_ids"]) and info["n_solver_constraints"] == len(ref["constraint_a"])
    assert info["last_scan"] == int(ref["alive"][-1]) and info["lifelong"] == 0 and info["n_supernodes"] >= 1 and info["n_running"] >= 1


def test_numpy_reader_equals_the_getters(good):
    ref, got = np.load(NPZ), session.read(KHMS)
    assert 20 not in got["ids"], "the removed node is still there"
    pairs = [("ids", "alive"), ("corrected", "poses"), ("ranges", "ranges"), ("score", "score"), ("localization_buffer", "localization_buffer"),
             ("adj", "adj"), ("node_ids", "node_ids"), ("node_poses", "node_poses"), ("constraint_a", "constraint_a"),
             ("constraint_b", "constraint_b"), ("constraint_z", "constraint_z"), ("constraint_information", "constraint_information")]
    for mine, theirs in pairs:
        a, b = got[mine], ref[theirs]
        assert a.shape == b.shape and a.dtype == b.dtype, (mine, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), mine
    assert np.array_equal(got["adj_count"][got["ids"]], ref["adj_count"]) and got["adj_count"][20] == 0 and got["out_count"][20] == 0
    assert got["n_scan_slots"] == int(ref["n_scan_slots"]) and got["n_edges"] == int(ref["n_edges"]) == int(got["out_count"].sum())
    assert got["laser"]["n_beams"] == 181 and got["params"]["loop_search_maximum_distance"] == 3.0 and got["params"]["scan_buffer_size"] == 10
    assert got["solver_gauge"] == {"has_first": 1, "first_id": 0, "was_constant_set": 1}
    assert got["solver_analysis"]["full_free_nodes"] > 0 and got["solver_analysis"]["full_flops"] > 0
    # the analysis cache names the free nodes of the last full dissection, each once (node 20 was removed after it: the next
    # analysis lets it drop out)
    sn = got["supernode_ids"]
    assert len(np.unique(sn)) == len(sn) == got["solver_analysis"]["full_free_nodes"] and 20 in sn and 0 not in sn
    assert got["last_scan"] == got["ids"][-1] and np.all(np.isin(got["running"], got["ids"]))


def test_truncated_files_are_refused(kartohip_lib, good, tmp_path):
    boundaries = [off for _, off, _ in session.sections(good)]
    lengths = [0, 3, 10, 23, 24, 24 + 24 * 5 + 7, boundaries[0] - 1] + [b - 1 for b in boundaries[1:]] + [len(good) - 1]
    assert len(set(lengths)) == len(lengths) == 18
    for n in lengths:
        p = tmp_path / f"cut_{n}.khms"
        p.write_bytes(good[:n])
        for rc, text in (_info_status(p), _load_status(p)):
            assert rc == capi.KH_ERR_IO and text.startswith("session file: "), (n, rc, text)
        with pytest.raises(session.SessionFormatError):
            session.read(p)


def test_damaged_files_are_refused(kartohip_lib, good, tmp_path):
    stat_off = dict((t, o) for t, o, _ in session.sections(good))["STAT"]
    n_slots, n_alive = struct.unpack_from("<qq", good, stat_off)
    payload = dict((t, o) for t, o, _ in session.sections(good))["RNGS"] + 1001

    def patched(at, raw):
        return good[:at] + raw + good[at + len(raw):]

    cases = {
        "missing": None,
        "magic": patched(0, b"KHMT"),
        "version": patched(4, struct.pack("<I", 2)),
        "payload_byte": patched(payload, bytes([good[payload] ^ 0x10])),
        "payload_byte_in_the_table": patched(24 + 8, bytes([good[24 + 8] ^ 0x01])),
        "file_size_field": patched(8, struct.pack("<Q", len(good) + 8)),
        # counts beyond what the file can hold, behind a checksum that is right again
        "scan_count": _with_checksum(patched(stat_off + 8, struct.pack("<q", n_alive + 1))),
        "scan_count_huge": _with_checksum(patched(stat_off + 8, struct.pack("<q", 1 << 40))),
        "slot_count_huge": _with_checksum(patched(stat_off, struct.pack("<qq", 1 << 30, n_alive))),
        "scan_count_negative": _with_checksum(patched(stat_off + 8, struct.pack("<q", -1))),
        "beam_count": _with_checksum(patched(dict((t, o) for t, o, _ in session.sections(good))["LASR"], struct.pack("<q", 182))),
        "node_count_huge": _with_checksum(patched(dict((t, o) for t, o, _ in session.sections(good))["SNOD"], struct.pack("<q", (1 << 62) + 5))),
        "constraint_count": _with_checksum(patched(dict((t, o) for t, o, _ in session.sections(good))["SCON"], struct.pack("<q", 1 << 33))),
        "supernode_count": _with_checksum(patched(dict((t, o) for t, o, _ in session.sections(good))["SANA"], struct.pack("<q", 1 << 50))),
        "last_scan_removed": _with_checksum(patched(stat_off + 24, struct.pack("<q", 20))),
    }
    texts = {}
    for name, data in cases.items():
        p = tmp_path / f"{name}.khms"
        if data is not None:
            assert len(data) == len(good) and data != good
            p.write_bytes(data)
        for rc, text in (_info_status(p), _load_status(p)):
            assert rc == capi.KH_ERR_IO and text.startswith("session file: "), (name, rc, text)
        texts[name] = text
    assert "magic" in texts["magic"] and "version" in texts["version"] and "checksum" in texts["payload_byte"]
    assert "checksum" in texts["payload_byte_in_the_table"] and "counts do not fit" in texts["scan_count"]
    # the untouched file still passes
    assert _info_status(KHMS)[0] == capi.KH_OK


def test_load_without_a_device_is_no_device_after_validation(kartohip_lib, tmp_path, good):
    rc, text = _load_status(KHMS)
    # (where a GPU is present the same call loads the session)
    assert rc == (capi.KH_OK if capi.lib().kh_device_count() > 0 else capi.KH_ERR_NO_DEVICE), (rc, text)
    bad = tmp_path / "bad.khms"
    bad.write_bytes(good[:-1])
    assert _load_status(bad)[0] == capi.KH_ERR_IO              # validation comes first


def test_argument_checks(kartohip_lib):
    L = capi.lib()
    h = C.c_void_p()
    assert L.kh_mapper_load(KHMS.encode(), np.zeros(1, dtype=np.int32), 0, 32, C.byref(h)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_load(KHMS.encode(), np.zeros(1, dtype=np.int32), 1, 0, C.byref(h)) == capi.KH_ERR_INVALID_ARG
    assert L.kh_session_info(KHMS.encode(), None) == capi.KH_ERR_INVALID_ARG
    assert L.kh_mapper_save(None, b"/tmp/never.khms") == capi.KH_ERR_INVALID_ARG
