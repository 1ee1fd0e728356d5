"""Host-side mirror of karto::Mapper's processing entry points (lib/karto_sdk/src/Mapper.cpp: Process :2679-2748, and the
localization mode's ProcessLocalization, ProcessAgainstNodesNearBy, ProcessAgainstNode / ProcessAtDock, ClearLocalizationBuffer) over the mapper
front end of libkartohip.so (kh_mapper_*): a ROS-free way to replay a scan queue end to end on the GPU.

    mapper = Mapper(laser, loop_search_maximum_distance=3.0)        # parameters of config/mapper_params_offline.yaml
    accepted, pose, cov = mapper.Process(ranges, odometric_pose, time)
    poses = mapper.poses()

Nothing here computes: every call lands in the library."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import capi


Hypothesis = namedtuple("Hypothesis", "index seed_scan heading coarse_mean coarse_cov coarse_response fine_mean fine_cov fine_response robot_pose")


class Mapper:
    def __init__(self, laser, device: int = 0, max_candidates: int = 32, log_path: str = None, devices=None, **params):
        """laser: anything with n_beams, min_angle, ang_res, min_range, max_range, range_threshold (synth.Laser);
        params: fields of kh_mapper_params to override (AS STORED by karto::Mapper: variances squared);
        devices: device list of kh_mapper_create_on_devices (candidate batches dealt over one matcher pair per entry; the
        same device may be listed more than once), default [device]."""
        p = capi.KhMapperParams()
        capi.lib().kh_mapper_params_default(C.byref(p))
        match_fields = {k for k, _ in capi.KhMatchParams._fields_}
        for k, v in params.items():
            if k in match_fields:
                setattr(p.match, k, v)
            elif hasattr(p, k):
                setattr(p, k, v)
            else:
                raise KeyError(k)
        off = tuple(getattr(laser, "offset", (0.0, 0.0, 0.0)))      # where the sensor sits on the robot (x, y, heading)
        L = capi.KhLaser(laser.n_beams, laser.min_angle, laser.ang_res, laser.min_range, laser.max_range, laser.range_threshold,
                         off[0], off[1], off[2])
        self._h = C.c_void_p()
        devs = np.asarray([device] if devices is None else list(devices), dtype=np.int32)
        capi.check(capi.lib().kh_mapper_create_on_devices(C.byref(p), C.byref(L), devs, len(devs), max_candidates, C.byref(self._h)),
                   "kh_mapper_create_on_devices")
        self.n_beams = laser.n_beams
        self._start = None
        if log_path:
            capi.check(capi.lib().kh_mapper_set_log(self._h, log_path.encode()), "kh_mapper_set_log")

    START_MODES = ("first_node", "given_pose", "localize_at_pose")

    @classmethod
    def load(cls, path, devices=None, max_candidates: int = 32, start: str = None, pose=None, log_path: str = None):
        """kh_mapper_load: the mapper a session file (Mapper.save) describes, ready to continue the run it was saved from.
        start: how the FIRST Process / ProcessLocalization call after the load enters, as slam_toolbox's addScan does after
        deserializePoseGraph (slam_toolbox_common.cpp:815-834, 1059-1076; slam_toolbox_localization.cpp:184-209):
        "first_node" = ProcessAtDock, "given_pose" = ProcessAgainstNodesNearBy with the scan's odometric pose set to `pose`,
        "localize_at_pose" = the same with the scan entering the localization buffer; every later call is the plain one.
        None continues where the saved run stopped."""
        if start is not None and start not in cls.START_MODES:
            raise ValueError(f"start must be one of {cls.START_MODES}")
        if start in ("given_pose", "localize_at_pose") and pose is None:
            raise ValueError(f"start={start!r} needs a pose")
        from . import session
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self._start = None
        devs = np.asarray([0] if devices is None else list(devices), dtype=np.int32)
        capi.check(capi.lib().kh_mapper_load(str(path).encode(), devs, len(devs), max_candidates, C.byref(self._h)), "kh_mapper_load")
        self.n_beams = session.info(path)["n_beams"]
        if start is not None:
            self._start = (start, None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).copy())
        if log_path:
            capi.check(capi.lib().kh_mapper_set_log(self._h, log_path.encode()), "kh_mapper_set_log")
        return self

    def save(self, path):
        """kh_mapper_save: everything the continuation of the run depends on, as one session file"""
        capi.check(capi.lib().kh_mapper_save(self._h, str(path).encode()), "kh_mapper_save")

    def build_map(self, resolution: float = 0.05, min_pass_through: int = 2, occupancy_threshold: float = 0.1):
        """kh_mapper_build_map: OccupancyGrid::CreateFromScans over the scans still in the map, traced from their resident copies.
        Returns an occupancy_grid.OccupancyGrid (cells / counters / width / height / offset)."""
        from .occupancy_grid import OccupancyGrid
        h = C.c_void_p()
        capi.check(capi.lib().kh_mapper_build_map(self._h, float(resolution), int(min_pass_through), float(occupancy_threshold), C.byref(h)),
                   "kh_mapper_build_map")
        return OccupancyGrid.from_handle(h, resolution)

    def live_map(self, resolution: float = 0.05, anchor=None, rebuild_fraction: float = None):
        """kh_live_map_create: an occupancy map that stays on the device next to this mapper and is brought up to date by the scans
        that entered, left or moved since its last update (live_map.LiveMap).  anchor None = the offset build_map would choose now;
        rebuild_fraction None = the library's default.  Close the live map before the mapper."""
        from .live_map import LiveMap
        return LiveMap(self, resolution, anchor, rebuild_fraction)

    def set_scan_pose(self, scan_id: int, corrected_pose):
        """kh_mapper_set_scan_pose: LocalizedRangeScan::SetCorrectedPose + Update of one scan (the solver is not told)"""
        capi.check(capi.lib().kh_mapper_set_scan_pose(self._h, int(scan_id), np.ascontiguousarray(corrected_pose, dtype=np.float64)),
                   "kh_mapper_set_scan_pose")

    def map_stats(self) -> dict:
        """counters of build_map: calls, scans traced / point uploads / range uploads of the last call, and the two totals"""
        out = np.zeros(6, dtype=np.int64)
        capi.check(capi.lib().kh_mapper_map_stats(self._h, out), "kh_mapper_map_stats")
        return dict(zip(("calls", "scans_traced", "point_uploads", "range_uploads", "point_uploads_total", "range_uploads_total"), out.tolist()))

    def relocalize(self, ranges, cap: int = 64, **params):
        """kh_mapper_relocalize: where in the map this scan was taken, without a pose guess.  params: fields of
        kh_relocalize_params (seed_spacing, n_headings, max_base, top_k, center_xy, radius) over the defaults of this mapper's
        parameters.  Returns (hypotheses, summary): the accepted hypotheses, best first, as Hypothesis records -- robot_pose is what
        ProcessAgainstNodesNearBy takes -- and the totals as a dict.  The mapper is left as it was."""
        ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        assert ranges.shape == (self.n_beams,)
        p = capi.KhRelocalizeParams()
        capi.lib().kh_relocalize_params_default(C.byref(self.params()), C.byref(p))
        for k, v in params.items():
            if k == "center_xy":
                p.center_xy[0], p.center_xy[1] = float(v[0]), float(v[1])
            elif k != "pad" and hasattr(p, k):
                setattr(p, k, v)
            else:
                raise KeyError(k)
        out = (capi.KhRelocalizeHyp * max(1, int(cap)))()
        summary = capi.KhRelocalizeSummary()
        capi.check(capi.lib().kh_mapper_relocalize(self._h, ranges.ctypes.data, C.byref(p), out, int(cap), C.byref(summary)), "kh_mapper_relocalize")
        hyps = [Hypothesis(h.index, h.seed_scan, h.heading, np.array(h.coarse_mean), np.array(h.coarse_cov).reshape(3, 3), h.coarse_response,
                           np.array(h.fine_mean), np.array(h.fine_cov).reshape(3, 3), h.fine_response, np.array(h.robot_pose))
                for h in out[:summary.n_returned]]
        return hyps, {k: getattr(summary, k) for k, _ in capi.KhRelocalizeSummary._fields_}

    def params(self):
        """the kh_mapper_params this mapper was made with"""
        p = capi.KhMapperParams()
        capi.check(capi.lib().kh_mapper_get_params(self._h, C.byref(p)), "kh_mapper_get_params")
        return p

    def _first_after_load(self, ranges, time):
        """the entry the first scan after a load goes through when a start mode was asked for; None = none pending"""
        if self._start is None:
            return None
        (start, pose), self._start = self._start, None
        if start == "first_node":
            return lambda odom: self.ProcessAtDock(ranges, odom, time)
        return lambda odom: self.ProcessAgainstNodesNearBy(ranges, pose, time, add_to_localization_buffer=(start == "localize_at_pose"))

    def Process(self, ranges, odometric_pose, time: float = 0.0):
        first = self._first_after_load(ranges, time)
        if first is not None:
            return first(odometric_pose)
        ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        assert ranges.shape == (self.n_beams,)
        acc = C.c_int32(0)
        pose, cov = np.zeros(3), np.zeros(9)
        capi.check(capi.lib().kh_mapper_process(self._h, ranges, np.ascontiguousarray(odometric_pose, dtype=np.float64), float(time),
                                                C.byref(acc), pose, cov), "kh_mapper_process")
        return bool(acc.value), pose, cov.reshape(3, 3)

    def _entry(self, fn, name, ranges, odometric_pose, time, *extra):
        ranges = np.ascontiguousarray(ranges, dtype=np.float64)
        assert ranges.shape == (self.n_beams,)
        odom = np.ascontiguousarray(odometric_pose, dtype=np.float64)
        acc = C.c_int32(0)
        pose, cov = np.zeros(3), np.zeros(9)
        capi.check(fn(self._h, ranges.ctypes.data, odom.ctypes.data, float(time), *extra, C.byref(acc), pose.ctypes.data, cov.ctypes.data), name)
        return bool(acc.value), pose, cov.reshape(3, 3)

    def ProcessLocalization(self, ranges, odometric_pose, time: float = 0.0):
        """Mapper::ProcessLocalization (Mapper.cpp:2831-2909): Process, then the scan enters the rolling buffer and the scan
        scan_buffer_size accepted scans back leaves the graph"""
        first = self._first_after_load(ranges, time)
        if first is not None:
            return first(odometric_pose)
        return self._entry(capi.lib().kh_mapper_process_localization, "kh_mapper_process_localization", ranges, odometric_pose, time)

    def ProcessAgainstNodesNearBy(self, ranges, odometric_pose, time: float = 0.0, add_to_localization_buffer: bool = False):
        """Mapper::ProcessAgainstNodesNearBy (Mapper.cpp:2751-2829): matched against the node nearest to the odometric pose"""
        return self._entry(capi.lib().kh_mapper_process_against_nodes_near_by, "kh_mapper_process_against_nodes_near_by", ranges,
                           odometric_pose, time, int(bool(add_to_localization_buffer)))

    def ProcessAgainstNode(self, ranges, odometric_pose, node_id: int, time: float = 0.0):
        """Mapper::ProcessAgainstNode (Mapper.cpp:3023-3096)"""
        return self._entry(capi.lib().kh_mapper_process_against_node, "kh_mapper_process_against_node", ranges, odometric_pose, time,
                           int(node_id))

    def ProcessAtDock(self, ranges, odometric_pose, time: float = 0.0):
        """Mapper::ProcessAtDock (Mapper.cpp:3098-3102): ProcessAgainstNode with the first node"""
        return self.ProcessAgainstNode(ranges, odometric_pose, 0, time)

    def ClearLocalizationBuffer(self):
        """Mapper::ClearLocalizationBuffer (Mapper.cpp:2939-2962)"""
        capi.check(capi.lib().kh_mapper_clear_localization_buffer(self._h), "kh_mapper_clear_localization_buffer")

    def localization_buffer(self) -> np.ndarray:
        """ids of the scans in the rolling buffer, oldest first"""
        n = C.c_int32(0)
        capi.check(capi.lib().kh_mapper_localization_buffer(self._h, None, 0, C.byref(n)), "kh_mapper_localization_buffer")
        ids = np.zeros(max(1, n.value), dtype=np.int32)
        capi.check(capi.lib().kh_mapper_localization_buffer(self._h, ids.ctypes.data, ids.size, C.byref(n)), "kh_mapper_localization_buffer")
        return ids[:n.value]

    def num_scans(self) -> int:
        return capi.lib().kh_mapper_num_scans(self._h)

    def num_edges(self) -> int:
        return capi.lib().kh_mapper_num_edges(self._h)

    def poses(self) -> np.ndarray:
        out = np.zeros((self.num_scans(), 3))
        if out.size:
            capi.check(capi.lib().kh_mapper_get_poses(self._h, out.reshape(-1)), "kh_mapper_get_poses")
        return out

    def scan(self, index: int):
        """(kh_scan, kh_scan_box) views of scan `index`: what the occupancy grid and the lifelong scoring read"""
        s, b = capi.KhScan(), capi.KhScanBox()
        capi.check(capi.lib().kh_mapper_get_scan(self._h, index, C.byref(s), C.byref(b)), "kh_mapper_get_scan")
        return s, b

    def adjacency(self, scan_id: int) -> np.ndarray:
        """Vertex::GetAdjacentVertices of the scan's vertex, in the reference's order"""
        n = C.c_int32(0)
        out = np.zeros(64, dtype=np.int32)
        capi.check(capi.lib().kh_mapper_get_adjacency(self._h, int(scan_id), out, out.size, C.byref(n)), "kh_mapper_get_adjacency")
        if n.value > out.size:
            out = np.zeros(n.value, dtype=np.int32)
            capi.check(capi.lib().kh_mapper_get_adjacency(self._h, int(scan_id), out, out.size, C.byref(n)), "kh_mapper_get_adjacency")
        return out[:n.value]

    def SetNodeScore(self, scan_id: int, score: float):
        """Vertex::SetScore (LifelongSlamToolbox::updateScoresSlamGraph)"""
        capi.check(capi.lib().kh_mapper_set_node_score(self._h, int(scan_id), float(score)), "kh_mapper_set_node_score")

    def RemoveNode(self, scan_id: int):
        """Mapper::RemoveNodeFromGraph + MapperSensorManager::RemoveScan (what lifelong mode does to a decayed node)"""
        capi.check(capi.lib().kh_mapper_remove_node(self._h, int(scan_id)), "kh_mapper_remove_node")

    def MarginalizeNodes(self, scan_ids):
        """kh_mapper_marginalize_nodes: the scans leave like RemoveNode, but their constraints are handed on to their neighbours
        (HipSpaSolver.MarginalizeNodes on the mapper's solver, mirrored in the mapper's edges)"""
        idv = np.ascontiguousarray(scan_ids, dtype=np.int32).reshape(-1)
        capi.check(capi.lib().kh_mapper_marginalize_nodes(self._h, idv.size, idv.ctypes.data_as(C.c_void_p)), "kh_mapper_marginalize_nodes")

    def SetRemovalMode(self, marginalize: bool):
        """how node decay removes a scan: False the reference's plain removal (default), True marginalizing removal.  Not stored
        in a session: set it again after load."""
        mode = capi.KH_REMOVE_MARGINALIZE if marginalize else capi.KH_REMOVE_PLAIN
        capi.check(capi.lib().kh_mapper_set_removal_mode(self._h, mode), "kh_mapper_set_removal_mode")

    def SetLifelong(self, enabled: bool = True, **decay):
        """LifelongSlamToolbox::evaluateNodeDepreciation after every accepted scan; decay = kh_decay_params overrides"""
        if not enabled:
            capi.check(capi.lib().kh_mapper_set_lifelong(self._h, None), "kh_mapper_set_lifelong")
            return
        p = capi.KhDecayParams()
        capi.lib().kh_decay_params_default(C.byref(p))
        for k, v in decay.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        capi.check(capi.lib().kh_mapper_set_lifelong(self._h, C.byref(p)), "kh_mapper_set_lifelong")

    def alive(self) -> np.ndarray:
        ids = np.zeros(max(1, capi.lib().kh_mapper_num_alive(self._h)), dtype=np.int32)
        capi.check(capi.lib().kh_mapper_get_alive(self._h, ids), "kh_mapper_get_alive")
        return ids[:capi.lib().kh_mapper_num_alive(self._h)]

    def covariances(self, ids=None) -> np.ndarray:
        """(n, 3, 3): graph-aware covariance of the listed scans' poses (None: every solver node, insertion order); computed by
        the solver on the first call after the graph or a pose has changed.  `cov_summary` holds the summary of the computation
        this call ran (all zeros when it ran none)."""
        L = capi.lib()
        if ids is None:
            n, idp = L.kh_spa_num_nodes(L.kh_mapper_solver(self._h)), None
        else:
            idv = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
            n, idp = idv.size, idv.ctypes.data_as(C.c_void_p)
        out = np.zeros((max(n, 1), 3, 3))
        s = capi.KhSpaCovSummary()
        rc = L.kh_mapper_get_covariances(self._h, n, idp, out.ctypes.data_as(C.c_void_p), C.byref(s))
        self.cov_summary = {k: getattr(s, k) for k, _ in capi.KhSpaCovSummary._fields_ if k != "pad"}
        capi.check(rc, "kh_mapper_get_covariances")
        return out[:n]

    def relative_covariances(self, ref, ids=None) -> np.ndarray:
        """(n, 3, 3): covariance of the listed scans' poses expressed in the frame of scan `ref` (None: every solver node,
        insertion order), from the graph as a whole: kh_mapper_get_relative_covariances.  The column of `ref` is computed only
        when it is not resident or is stale; `cov_columns_summary` holds the summary of the computation this call ran (all zeros
        when it ran none)."""
        L = capi.lib()
        if ids is None:
            n, idp = L.kh_spa_num_nodes(L.kh_mapper_solver(self._h)), None
        else:
            idv = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
            n, idp = idv.size, idv.ctypes.data_as(C.c_void_p)
        out = np.zeros((max(n, 1), 3, 3))
        s = capi.KhSpaCovColumnsSummary()
        rc = L.kh_mapper_get_relative_covariances(self._h, int(ref), n, idp, out.ctypes.data_as(C.c_void_p), C.byref(s))
        self.cov_columns_summary = {k: getattr(s, k) for k, _ in capi.KhSpaCovColumnsSummary._fields_ if k != "cov"}
        self.cov_columns_summary["cov"] = {k: getattr(s.cov, k) for k, _ in capi.KhSpaCovSummary._fields_ if k != "pad"}
        capi.check(rc, "kh_mapper_get_relative_covariances")
        return out[:n]

    def difference_covariances(self, ref, ids=None) -> np.ndarray:
        """(n, 3, 3): world-frame covariance of x_i - x_ref for the listed scans (None: every solver node, insertion order):
        kh_mapper_get_difference_covariances, lazy like relative_covariances."""
        L = capi.lib()
        if ids is None:
            n, idp = L.kh_spa_num_nodes(L.kh_mapper_solver(self._h)), None
        else:
            idv = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
            n, idp = idv.size, idv.ctypes.data_as(C.c_void_p)
        out = np.zeros((max(n, 1), 3, 3))
        s = capi.KhSpaCovColumnsSummary()
        rc = L.kh_mapper_get_difference_covariances(self._h, int(ref), n, idp, out.ctypes.data_as(C.c_void_p), C.byref(s))
        self.cov_columns_summary = {k: getattr(s, k) for k, _ in capi.KhSpaCovColumnsSummary._fields_ if k != "cov"}
        self.cov_columns_summary["cov"] = {k: getattr(s.cov, k) for k, _ in capi.KhSpaCovSummary._fields_ if k != "pad"}
        capi.check(rc, "kh_mapper_get_difference_covariances")
        return out[:n]

    def SetLoopGate(self, enabled: bool = True, **params):
        """kh_mapper_set_loop_gate: the loop search gated by the pose graph's covariances.  params: fields of
        kh_loop_gate_params (refresh_scans, chi2_position, chi2_jump, covariance_scale, max_reach) over the defaults of this
        mapper's parameters.  Not stored in a session: set it again after load."""
        g = capi.KhLoopGateParams()
        capi.lib().kh_loop_gate_params_default(C.byref(self.params()), C.byref(g))
        for k, v in params.items():
            if k == "enabled" or not hasattr(g, k):
                raise KeyError(k)
            setattr(g, k, v)
        g.enabled = 1 if enabled else 0
        capi.check(capi.lib().kh_mapper_set_loop_gate(self._h, C.byref(g)), "kh_mapper_set_loop_gate")

    def loop_gate(self) -> dict:
        g = capi.KhLoopGateParams()
        capi.check(capi.lib().kh_mapper_get_loop_gate(self._h, C.byref(g)), "kh_mapper_get_loop_gate")
        return {k: getattr(g, k) for k, _ in capi.KhLoopGateParams._fields_}

    def loop_gate_stats(self) -> dict:
        """column passes run for the gate and their wall time, searches left ungated, chains the jump test rejected, the largest
        semi-axis (m) a prepared row had"""
        st = capi.KhLoopGateStats()
        capi.check(capi.lib().kh_mapper_get_loop_gate_stats(self._h, C.byref(st)), "kh_mapper_get_loop_gate_stats")
        return {k: getattr(st, k) for k, _ in capi.KhLoopGateStats._fields_}

    # ---- single-edge edits, constraint audit, outlier rejection ----
    def AddEdge(self, from_scan: int, to_scan: int, mean_sensor_pose, covariance, correct: bool = True):
        """kh_mapper_add_edge: a manual loop closure.  mean_sensor_pose: the sensor pose of `to_scan` the constraint asserts."""
        mean = np.ascontiguousarray(mean_sensor_pose, dtype=np.float64).reshape(3)
        cov = np.ascontiguousarray(covariance, dtype=np.float64).reshape(9)
        capi.check(capi.lib().kh_mapper_add_edge(self._h, int(from_scan), int(to_scan), mean.ctypes.data_as(C.c_void_p),
                                                 cov.ctypes.data_as(C.c_void_p), 1 if correct else 0), "kh_mapper_add_edge")

    def RemoveEdge(self, from_scan: int, to_scan: int):
        """kh_mapper_remove_edge: KartoHipError (KH_ERR_NOT_FOUND) when there is no edge with that source and target"""
        capi.check(capi.lib().kh_mapper_remove_edge(self._h, int(from_scan), int(to_scan)), "kh_mapper_remove_edge")

    def CorrectPoses(self):
        capi.check(capi.lib().kh_mapper_correct_poses(self._h), "kh_mapper_correct_poses")

    def audit(self, min_redundancy: float = 1e-6) -> np.ndarray:
        """kh_mapper_audit: the leave-one-out test of every constraint of the graph (capi.AUDIT_DTYPE, ids are scan ids)"""
        L = capi.lib()
        cap = max(L.kh_spa_num_constraints(L.kh_mapper_solver(self._h)), 1)
        out = np.zeros(cap, dtype=capi.AUDIT_DTYPE)
        n, s = C.c_int32(0), capi.KhSpaAuditSummary()
        rc = L.kh_mapper_audit(self._h, float(min_redundancy), out.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(s))
        self.audit_summary = capi.audit_summary_dict(s)
        capi.check(rc, "kh_mapper_audit")
        return out[:n.value]

    def RejectOutliers(self, cap: int = 64, **params) -> np.ndarray:
        """kh_mapper_reject_outliers: rounds of solve + audit, each removing the newest of the verifiable non-odometry constraints
        tied for the largest chi2_loo while that exceeds `chi2`.  params: fields of kh_reject_params over its defaults.  Returns
        the records of the removed constraints as audited in the round that removed them; the summary is kept as `reject_summary`."""
        L = capi.lib()
        p = capi.KhRejectParams()
        L.kh_reject_params_default(C.byref(p))
        for k, v in params.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        out = np.zeros(max(int(cap), 1), dtype=capi.AUDIT_DTYPE)
        s = capi.KhRejectSummary()
        rc = L.kh_mapper_reject_outliers(self._h, C.byref(p), out.ctypes.data_as(C.c_void_p), int(cap), C.byref(s))
        self.reject_summary = {k: getattr(s, k) for k, _ in capi.KhRejectSummary._fields_}
        capi.check(rc, "kh_mapper_reject_outliers")
        return out[:s.n_removed]

    def stats(self) -> dict:
        st = capi.KhMapperStats()
        capi.check(capi.lib().kh_mapper_get_stats(self._h, C.byref(st)), "kh_mapper_get_stats")
        return {k: getattr(st, k) for k, _ in capi.KhMapperStats._fields_}

    def set_log(self, path):
        capi.check(capi.lib().kh_mapper_set_log(self._h, path.encode() if path else None), "kh_mapper_set_log")

    def close(self):
        if self._h:
            capi.lib().kh_mapper_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
