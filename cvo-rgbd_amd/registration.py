"""Python mirror of the reference's registration objects.

``Cvo`` ~ cvo::cvo (ref cpp/rkhs_registration/include/cvo.hpp:55-193),
``Acvo`` ~ acvo::acvo (ref include/adaptive_cvo.hpp:57-196): same members
(init, iter, transform, prev_transform, accum_transform) and methods
(set_pcd, align, run_cvo), the point cloud arriving as arrays instead of
cv::Mat images (the image front end is outside this back end).
All computation goes through the HIP C-ABI; nothing here has a CPU path.
"""
import numpy as np

from . import capi


def pose_grid(R0, T0, rotations, translations):
    """Candidate poses around (R0, T0) for align(init_candidates=...): every (R0 @ dR, T0 + dT) of the two lists, in
    row-major product order (rotations outer, translations inner).  Returns (Rs, Ts): float32 arrays of shape
    (len(rotations) * len(translations), 3, 3) and (..., 3); the products and sums are formed in float64."""
    R0 = np.asarray(R0, np.float64).reshape(3, 3)
    T0 = np.asarray(T0, np.float64).reshape(3)
    rot = np.asarray(rotations, np.float64).reshape(-1, 3, 3)
    tr = np.asarray(translations, np.float64).reshape(-1, 3)
    Rs = np.repeat(R0 @ rot, len(tr), axis=0)
    Ts = np.tile(T0 + tr, (len(rot), 1))
    return Rs.astype(np.float32), Ts.astype(np.float32)


class _Registration:
    MODE = capi.MODE_CVO

    def __init__(self, device=0, stream=None, params=None, graph_capture=None):
        self.params = params if params is not None else capi.default_params(self.MODE)
        self.ctx = capi.Context(self.params, device=device, stream=stream, graph_capture=graph_capture)
        self.state = capi.init_state(self.params)
        self.init = False
        self.iter = 0
        self.transform = np.eye(4, dtype=np.float32)
        self.prev_transform = np.eye(4, dtype=np.float32)
        self.accum_transform = np.eye(4, dtype=np.float32)
        self.num_iterations = 0
        self.trace = []
        self.hessian = None   # align(hessian=True) publishes the pose Hessian here
        self.score = None     # align(score=...) publishes the pose score here
        self.scores = []      # run_sequence(score=...): one pose score per pair
        self.matches = None   # align(matches=...) publishes the per-point matches here
        self.matches_list = []   # run_sequence(matches=...): one capi.PoseMatches per pair
        self.scan = None      # align(init_candidates=...) publishes the scan of the starting poses here
        self._have_moving = False

    def _publish(self):
        s = self.state
        self.transform = np.array(s.transform, np.float32).reshape(4, 4)
        self.prev_transform = np.array(s.prev_transform, np.float32).reshape(4, 4)
        self.accum_transform = np.array(s.accum_transform, np.float32).reshape(4, 4)
        self.iter = int(s.iter)

    def set_pcd(self, positions, features, layout=capi.FEAT_ROWMAJOR):
        """ref src/cvo.cpp:319-357 (tail: hand the clouds to the back end)."""
        if not self.init:
            self.ctx.set_fixed(positions, features, layout)
            self.init = True
            return
        self.ctx.set_moving(positions, features, layout)
        self._have_moving = True

    def set_pcd_device(self, d_positions, d_features, n, layout=capi.FEAT_ROWMAJOR):
        """set_pcd with the cloud already in device memory (e.g. PcdGenerator.collect_device)."""
        if not self.init:
            self.ctx.set_fixed_device(d_positions, d_features, n, layout)
            self.init = True
            return
        self.ctx.set_moving_device(d_positions, d_features, n, layout)
        self._have_moving = True

    def run_cvo_device(self, d_positions, d_features, n, layout=capi.FEAT_ROWMAJOR, trace_cap=0, score=False, matches=False,
                       init_candidates=None, scan_ell=None):
        first = not self.init
        self.set_pcd_device(d_positions, d_features, n, layout)
        if not first:
            self.align(trace_cap=trace_cap, score=score, matches=matches, init_candidates=init_candidates, scan_ell=scan_ell)

    def align(self, trace_cap=0, hessian=False, score=False, matches=False, init_candidates=None, scan_ell=None):
        """ref src/cvo.cpp:361-420.

        init_candidates=(Rs, Ts): before the loop, score the pose the object carries and these candidate poses -- (n, 3, 3)
        and (n, 3), e.g. from pose_grid() -- in one call (capi.Context.pose_scan, include/cvo_hip.h cvo_hip_pose_scan) at
        ``scan_ell`` (default ``params.ell_init``), and start the loop from the one with the largest inner product.
        Index 0 of the scanned list is the carried pose, the candidates follow: by the scan's own measure the start is
        never worse than without it.  The scan is published as ``self.scan`` (a capi.PoseScan; ``best`` 0: the carried
        pose stayed, -1: no pose has a member and the carried pose stayed).  None: nothing changes, bit for bit.

        hessian=True: after the loop, evaluate the pose Hessian of the CVO objective at the final R, T and
        length scale (capi.Context.pose_hessian, include/cvo_hip.h cvo_hip_pose_hessian) before the moving
        cloud becomes the fixed one, and publish it as ``self.hessian`` (a capi.PoseHessian: f, g, H, nnz).
        -H is the information-like quantity of the registration; no noise model is implied.

        score=True: after the loop, score the registration at the final R, T (capi.Context.pose_score,
        include/cvo_hip.h cvo_hip_pose_score) at ``params.ell_init`` -- one fixed length scale per object, so
        that the scores of a sequence can be compared and each cloud's norm is computed once -- and publish it
        as ``self.score`` (a capi.PoseScore; cos_angle is the normalised inner product).  A float: score at
        that length scale.

        matches=True (or a length scale, as for score): after the loop, ask which points matched at the final R, T
        (capi.Context.pose_matches, include/cvo_hip.h cvo_hip_pose_matches) and publish the answer as
        ``self.matches`` (a capi.PoseMatches: per point of the fixed and of the moving cloud, in the caller's order,
        the support, the number of members and the best match in the other cloud).

        The registration itself is the same bit for bit with or without any of them."""
        if not self._have_moving:
            raise capi.CvoHipError("align(): set_pcd() must precede each align()")
        if init_candidates is not None:
            Rs, Ts = init_candidates
            st = self.state
            Rs = np.concatenate([np.array(st.R, np.float32).reshape(1, 3, 3), np.asarray(Rs, np.float32).reshape(-1, 3, 3)])
            Ts = np.concatenate([np.array(st.T, np.float32).reshape(1, 3), np.asarray(Ts, np.float32).reshape(-1, 3)])
            self.scan = self.ctx.pose_scan(Rs, Ts, self.params.ell_init if scan_ell is None else float(scan_ell))
            if self.scan.best > 0:
                st.R[:] = [float(v) for v in Rs[self.scan.best].ravel()]
                st.T[:] = [float(v) for v in Ts[self.scan.best]]
        self.num_iterations, self.trace = self.ctx.align(self.state, trace_cap=trace_cap)
        if hessian:
            s = self.state
            self.hessian = self.ctx.pose_hessian(np.array(s.R, np.float32), np.array(s.T, np.float32), s.ell)
        if score is not False and score is not None:
            s = self.state
            ell = self.params.ell_init if score is True else float(score)
            self.score = self.ctx.pose_score(np.array(s.R, np.float32), np.array(s.T, np.float32), ell)
        if matches is not False and matches is not None:
            s = self.state
            ell = self.params.ell_init if matches is True else float(matches)
            self.matches = self.ctx.pose_matches(np.array(s.R, np.float32), np.array(s.T, np.float32), ell)
        self.ctx.swap_moving_to_fixed()   # ptr_fixed_pcd = std::move(ptr_moving_pcd)
        self._have_moving = False
        self._publish()

    def run_cvo(self, positions, features, layout=capi.FEAT_ROWMAJOR, trace_cap=0, hessian=False, score=False, matches=False,
                init_candidates=None, scan_ell=None):
        """ref src/cvo.cpp:422-435 (hessian, score, matches, init_candidates, scan_ell: see align())."""
        if not self.init:
            self.set_pcd(positions, features, layout)
        else:
            self.set_pcd(positions, features, layout)
            self.align(trace_cap=trace_cap, hessian=hessian, score=score, matches=matches, init_candidates=init_candidates,
                       scan_ell=scan_ell)

    def run_sequence(self, frames, writer=None, trace_cap=0, hessian=False, score=False, matches=False):
        """The loop of the reference's drivers (ref src/cvo_main.cpp:36-66): every
        frame goes through run_cvo() and then gets a pose line of `accum_transform`
        in `writer` (a trajectory.TrajectoryWriter) -- the first frame too (the
        identity): `init` is already true after the first run_cvo()
        (ref cvo_main.cpp:52,58).  `frames` yields (name,
        positions, features).  Returns the per-pair iteration counts.  hessian=True: every
        pair's align() evaluates the pose Hessian (align()); the last one stays in ``self.hessian``.
        score=True (or a length scale): every pair is scored (align()) and ``self.scores`` holds one
        capi.PoseScore per pair of this call, in order.  matches=True (or a length scale): likewise
        ``self.matches_list`` holds one capi.PoseMatches per pair (fixed = the earlier frame of the pair)."""
        iters = []
        want_matches = matches is not False and matches is not None
        if want_matches:
            self.matches_list = []
        if score is not False and score is not None:
            self.scores = []
        for name, positions, features in frames:
            first = not self.init
            self.run_cvo(positions, features, trace_cap=trace_cap, hessian=hessian, score=score, matches=matches)
            if not first:
                iters.append(self.num_iterations)
                if want_matches:
                    self.matches_list.append(self.matches)
                if score is not False and score is not None:
                    self.scores.append(self.score)
            if writer is not None and self.init:
                writer.append(name, self.accum_transform)
        return iters

    def close(self):
        self.ctx.close()


class Cvo(_Registration):
    MODE = capi.MODE_CVO


class RkhsMatlab(_Registration):
    """The reference's MATLAB registration object (ref matlab/@rkhs_se3_registration/
    rkhs_se3_registration.m) on the same HIP kernels: linear colour inner
    product CI = 1e-5 <c_i, c_j>, squared-exponential kernel thresholded at 1e-3 on K
    alone, eps 5e-4 / 1e-4 (:10-28,40-73,125-127).  Unlike the C++ objects it starts every
    pair from R = I, T = 0, ell = 0.15 (:112-114).  Arithmetic is this library's float32
    per-pair contract, not MATLAB's float64: results agree with a float64 restatement
    (oracle/matlab_dense.py) to ~1e-5."""
    MODE = capi.MODE_MATLAB

    @staticmethod
    def features(rgb):
        """n x 3 colour bytes -> the n x 5 feature rows the kernels read (channels 0..2)."""
        f = np.zeros((len(rgb), 5), np.float32)
        f[:, :3] = np.asarray(rgb, np.float32)
        return f

    def register(self, fixed_xyz, fixed_rgb, moving_xyz, moving_rgb):
        """One pair as rgbddataset_rkhs.m drives the object (ref :30-75): returns the 4 x 4
        `tform` = [R' -R'T; 0 1] and the number of iterations."""
        self.state = capi.init_state(self.params)
        self.ctx.set_fixed(np.ascontiguousarray(fixed_xyz, np.float32), self.features(fixed_rgb))
        self.ctx.set_moving(np.ascontiguousarray(moving_xyz, np.float32), self.features(moving_rgb))
        self.init = True
        self._have_moving = True
        self.num_iterations, self.trace = self.ctx.align(self.state, trace_cap=0)
        self._have_moving = False
        self._publish()
        return self.transform.copy(), self.num_iterations


class Acvo(_Registration):
    MODE = capi.MODE_ACVO

    def function_inner_product(self, cloud_a, cloud_b, layout=capi.FEAT_ROWMAJOR):
        """ref include/adaptive_cvo.hpp:179, src/adaptive_cvo.cpp:385-439: the statistic between
        two arbitrary clouds -- (positions, features) each -- at the current length-scale.
        Registration state is untouched (a pending set_pcd() stays pending)."""
        return self.ctx.function_inner_product_clouds(self.state.ell, cloud_a[0], cloud_a[1],
                                                      cloud_b[0], cloud_b[1], layout)
