"""Python mirror of the candidate-enumeration part of karto::MapperGraph over the C ABI
(kh_graph_*): FindNearLinkedScans + FindPossibleLoopClosure for a batch of query scans on the GPU.  Same
argument meaning as the reference: positions are GetReferencePose(use_scan_barycenter) of the scans in
scan-list order, adjacency in Vertex::GetAdjacentVertices order."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class MapperGraphSearch:
    def __init__(self, device: int = 0):
        h = C.c_void_p()
        capi.check(capi.lib().kh_graph_create(device, C.byref(h)), "kh_graph_create")
        self._h = h
        self.n = 0

    def SetGraph(self, ref_xy, adj_ptr, adj_idx):
        ref_xy = np.ascontiguousarray(ref_xy, dtype=np.float64).reshape(-1, 2)
        adj_ptr = np.ascontiguousarray(adj_ptr, dtype=np.int32)
        adj_idx = np.ascontiguousarray(adj_idx, dtype=np.int32)
        if adj_idx.size == 0:
            adj_idx = np.zeros(1, dtype=np.int32)
        capi.check(capi.lib().kh_graph_set(self._h, ref_xy.shape[0], ref_xy.reshape(-1), adj_ptr, adj_idx), "kh_graph_set")
        self.n = ref_xy.shape[0]

    def SetPositions(self, ref_xy):
        """After CorrectPoses(): same topology, moved scans."""
        ref_xy = np.ascontiguousarray(ref_xy, dtype=np.float64).reshape(-1, 2)
        capi.check(capi.lib().kh_graph_set_positions(self._h, ref_xy.shape[0], ref_xy.reshape(-1)), "kh_graph_set_positions")

    def SetScanLimit(self, n_visit):
        """The candidate walks visit the first n_visit scans only (the reference's scan map size after removals); SetGraph
        resets it to n."""
        capi.check(capi.lib().kh_graph_set_scan_limit(self._h, int(n_visit)), "kh_graph_set_scan_limit")

    def AddEdge(self, scan_a, scan_b):
        capi.check(capi.lib().kh_graph_add_edge(self._h, int(scan_a), int(scan_b)), "kh_graph_add_edge")

    def SetPosition(self, scan, ref_xy):
        xy = np.ascontiguousarray(ref_xy, dtype=np.float64)[:2].copy()
        capi.check(capi.lib().kh_graph_set_position(self._h, int(scan), xy), "kh_graph_set_position")

    def FindPossibleLoopClosures(self, query_scans, loop_search_maximum_distance, loop_match_minimum_chain_size, starts=None):
        """-> list (one entry per query) of [(first, last), ...]: every chain successive
        MapperGraph::FindPossibleLoopClosure calls would return for that scan (Mapper.cpp:1960-2010); with `starts`, the
        calls of query i begin at rStartNum = starts[i] (kh_graph_find_loop_candidates_from)."""
        q = np.ascontiguousarray(query_scans, dtype=np.int32)
        if starts is not None:
            starts = np.ascontiguousarray(starts, dtype=np.int32)
            if starts.shape != q.shape:
                raise ValueError("one start per query")
        begin = np.zeros(q.size + 1, dtype=np.int32)
        cap = max(16, 4 * q.size)
        total = C.c_int32(0)
        while True:
            chains = np.zeros(2 * cap, dtype=np.int32)
            if starts is None:
                capi.check(capi.lib().kh_graph_find_loop_candidates(self._h, q.size, q, float(loop_search_maximum_distance),
                                                                    int(loop_match_minimum_chain_size), begin, chains, cap,
                                                                    C.byref(total)), "kh_graph_find_loop_candidates")
            else:
                capi.check(capi.lib().kh_graph_find_loop_candidates_from(self._h, q.size, q, starts.ctypes.data, float(loop_search_maximum_distance),
                                                                         int(loop_match_minimum_chain_size), begin, chains, cap,
                                                                         C.byref(total)), "kh_graph_find_loop_candidates_from")
            if total.value <= cap:
                break
            cap = total.value
        chains = chains.reshape(-1, 2)
        return [[(int(a), int(b)) for a, b in chains[begin[i]: begin[i + 1]]] for i in range(q.size)]

    def find_loop_candidates(self, query_scans, loop_search_maximum_distance, loop_match_minimum_chain_size, starts=None, gate=None,
                             chi2: float = 0.0):
        """FindPossibleLoopClosures with the covariance gate (kh_graph_find_loop_candidates_gated): gate is
        (n_queries, n_scans, 3, 3) -- per query and scan, in list order, the world-frame covariance of the scan's displacement from
        the query -- and chi2 the size of the ellipse the search disk is widened by.  gate=None is the ungated call."""
        if gate is None:
            return self.FindPossibleLoopClosures(query_scans, loop_search_maximum_distance, loop_match_minimum_chain_size, starts)
        q = np.ascontiguousarray(query_scans, dtype=np.int32)
        gate = np.ascontiguousarray(gate, dtype=np.float64)
        if gate.size != q.size * self.n * 9:
            raise ValueError("gate must hold 9 doubles per query and scan")
        startp = None
        if starts is not None:
            starts = np.ascontiguousarray(starts, dtype=np.int32)
            if starts.shape != q.shape:
                raise ValueError("one start per query")
            startp = starts.ctypes.data_as(C.c_void_p)
        begin = np.zeros(q.size + 1, dtype=np.int32)
        cap = max(16, 4 * q.size)
        total = C.c_int32(0)
        while True:
            chains = np.zeros(2 * cap, dtype=np.int32)
            capi.check(capi.lib().kh_graph_find_loop_candidates_gated(
                self._h, q.size, q.ctypes.data_as(C.c_void_p), startp, float(loop_search_maximum_distance), int(loop_match_minimum_chain_size),
                float(chi2), gate.ctypes.data_as(C.c_void_p), begin.ctypes.data_as(C.c_void_p), chains.ctypes.data_as(C.c_void_p), cap,
                C.byref(total)), "kh_graph_find_loop_candidates_gated")
            if total.value <= cap:
                break
            cap = total.value
        chains = chains.reshape(-1, 2)
        return [[(int(a), int(b)) for a, b in chains[begin[i]: begin[i + 1]]] for i in range(q.size)]

    def FindNearChains(self, query_scan, link_scan_maximum_distance):
        """MapperGraph::FindNearChains (Mapper.cpp:1683-1793) -> [(first, last), ...] in the reference's order."""
        cap = 64
        total = C.c_int32(0)
        while True:
            chains = np.zeros(2 * cap, dtype=np.int32)
            capi.check(capi.lib().kh_graph_find_near_chains(self._h, int(query_scan), float(link_scan_maximum_distance),
                                                            chains, cap, C.byref(total)), "kh_graph_find_near_chains")
            if total.value <= cap:
                break
            cap = total.value
        return [(int(a), int(b)) for a, b in chains.reshape(-1, 2)[:total.value]]

    def GetClosestScanToPose(self, scans, pose_xy):
        """MapperGraph::GetClosestScanToPose (Mapper.cpp:1563-1582); -1 for an empty list."""
        scans = np.ascontiguousarray(scans, dtype=np.int32)
        out = C.c_int32(-1)
        capi.check(capi.lib().kh_graph_closest_scan_to_pose(self._h, scans if scans.size else np.zeros(1, dtype=np.int32),
                                                            scans.size, np.ascontiguousarray(pose_xy, dtype=np.float64)[:2].copy(),
                                                            C.byref(out)), "kh_graph_closest_scan_to_pose")
        return out.value

    def SetPoses(self, pose_xy):
        """GetCorrectedPose() x, y of every vertex: the points the near-by queries measure to (after SetGraph, and again after
        CorrectPoses)."""
        pose_xy = np.ascontiguousarray(pose_xy, dtype=np.float64).reshape(-1, 2)
        capi.check(capi.lib().kh_graph_set_poses(self._h, pose_xy.shape[0], pose_xy.ctypes.data), "kh_graph_set_poses")

    def SetPose(self, scan, pose_xy):
        xy = np.ascontiguousarray(pose_xy, dtype=np.float64)[:2].copy()
        capi.check(capi.lib().kh_graph_set_pose(self._h, int(scan), xy.ctypes.data), "kh_graph_set_pose")

    def AppendScan(self, ref_xy, pose_xy):
        ref = np.ascontiguousarray(ref_xy, dtype=np.float64)[:2].copy()
        pose = np.ascontiguousarray(pose_xy, dtype=np.float64)[:2].copy()
        capi.check(capi.lib().kh_graph_append_scan_with_pose(self._h, ref.ctypes.data, pose.ctypes.data), "kh_graph_append_scan_with_pose")
        self.n += 1

    def FindNearByScan(self, query_xy):
        """MapperGraph::FindNearByScan (Mapper.cpp:1877-1912) for one pose (x, y) or a batch (q, 2) in one kernel launch
        -> (nearest, dist_sq): vertex index (-1 for an empty graph) and squared distance, scalars for one pose."""
        q = np.ascontiguousarray(query_xy, dtype=np.float64)
        single = q.ndim == 1
        q = np.ascontiguousarray(q.reshape(-1, q.shape[-1])[:, :2])
        nearest = np.full(q.shape[0], -1, dtype=np.int32)
        dist_sq = np.zeros(q.shape[0])
        capi.check(capi.lib().kh_graph_find_near_by_scan(self._h, q.shape[0], q.ctypes.data, nearest.ctypes.data, dist_sq.ctypes.data),
                   "kh_graph_find_near_by_scan")
        return (int(nearest[0]), float(dist_sq[0])) if single else (nearest, dist_sq)

    def FindNearByVertices(self, query_xy, max_distance):
        """MapperGraph::FindNearByVertices (Mapper.cpp:1837-1875): the vertices with SQUARED distance < max_distance (the
        reference's radiusSearch call, nanoflann.hpp:274), by ascending distance."""
        q = np.ascontiguousarray(query_xy, dtype=np.float64)[:2].copy()
        cap = 256
        total = C.c_int32(0)
        while True:
            out = np.zeros(cap, dtype=np.int32)
            capi.check(capi.lib().kh_graph_find_near_by_vertices(self._h, q.ctypes.data, float(max_distance), out.ctypes.data, cap,
                                                                 C.byref(total)), "kh_graph_find_near_by_vertices")
            if total.value <= cap:
                return out[:total.value]
            cap = total.value

    def RelocalizeCandidates(self, seed_spacing, base_radius, max_base=40, center_xy=None, radius=0.0):
        """kh_graph_relocalize_candidates over the store's poses -> (seeds, base_begin, base_idx): the vertex of lowest index of every
        cell of a lattice of side seed_spacing (inside the region, if one is given), and per seed the vertices within base_radius of it,
        at most max_base of them by the stride rule, in CSR form"""
        c = None if center_xy is None else np.ascontiguousarray(center_xy, dtype=np.float64)[:2].copy()
        cap_s, cap_b = 64, 1024
        n_s, n_b = C.c_int32(0), C.c_int32(0)
        while True:
            seeds, begin, idx = np.zeros(cap_s, dtype=np.int32), np.zeros(cap_s + 1, dtype=np.int32), np.zeros(cap_b, dtype=np.int32)
            capi.check(capi.lib().kh_graph_relocalize_candidates(self._h, float(seed_spacing), float(base_radius), int(max_base),
                                                                 None if c is None else c.ctypes.data, float(radius), seeds.ctypes.data, cap_s,
                                                                 C.byref(n_s), begin.ctypes.data, idx.ctypes.data, cap_b, C.byref(n_b)),
                       "kh_graph_relocalize_candidates")
            if n_s.value <= cap_s and n_b.value <= cap_b:
                return seeds[:n_s.value], begin[:n_s.value + 1], idx[:n_b.value]
            cap_s, cap_b = max(cap_s, n_s.value), max(cap_b, n_b.value)

    def last_relocalize_kernel_ms(self):
        return capi.lib().kh_graph_last_relocalize_kernel_ms(self._h)

    def last_kernel_ms(self):
        return capi.lib().kh_graph_last_kernel_ms(self._h)

    def last_near_by_kernel_ms(self):
        return capi.lib().kh_graph_last_near_by_kernel_ms(self._h)

    def close(self):
        if self._h:
            capi.lib().kh_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ComputeWeightedMean(means, covariances):
    """MapperGraph::ComputeWeightedMean (Mapper.cpp:1914-1958)."""
    means = np.ascontiguousarray(means, dtype=np.float64).reshape(-1, 3)
    covs = np.ascontiguousarray(covariances, dtype=np.float64).reshape(-1, 9)
    out = np.zeros(3)
    capi.check(capi.lib().kh_weighted_mean(means.shape[0], means.reshape(-1), covs.reshape(-1), out), "kh_weighted_mean")
    return out
