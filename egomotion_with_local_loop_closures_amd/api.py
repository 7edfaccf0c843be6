"""Thin Python view of the C ABI (numpy in / numpy out). All compute happens in libellc_hip.so on the GPU."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import EllcConfig, EllcHypotheses, EllcAlignQuality, EllcMapPoint, EllcMapFilter, EllcDepthConsistency, EllcSim3Params, EllcSim3Normal, EllcLightNormal, EllcLightParams, EllcRefineParams, EllcRefineStats, REFINE_STATUS, EllcSweepParams, EllcSweepStats, SWEEP_STATUS, SWEEP_STATS_FIELDS, EllcCullParams, EllcCullStats, CULL_STATUS, CULL_STATS_FIELDS, EllcJointParams, EllcJointNormal, EllcJointApplyStats, JOINT_STATUS, JOINT_MAX_VIEWS, EllcAbsorbParams, EllcAbsorbStats, ABSORB_STATS_FIELDS, EllcTrialPropagation, EllcTrialPropagationLit, EllcError, MAX_LEVELS

MODE_FCA = 0
MODE_ICA = 1
ARITH_EXACT = 0
ARITH_FAST = 1
ERR_CAPACITY = -5
MAP_POINT_DTYPE = np.dtype(EllcMapPoint)   # x y z var (f32), px py (u16), intensity support (u8), source (u16): 24 bytes
LIGHT_NORMAL_DTYPE = np.dtype(EllcLightNormal)   # sum_w, sum_w_s, sum_w_t, sum_w_ss, sum_w_st, sum_w_tt, chi2_photo (f64), four int32 counts: 72 bytes
TRIAL_LIT_DTYPE = np.dtype(EllcTrialPropagationLit)   # ellc_trial_propagation's 48 bytes, sum_s, sum_t, sum_ss, sum_st, sum_tt (f64), n_fit, reserved2 (int32): 96 bytes
SIM3_NORMAL_DTYPE = np.dtype(EllcSim3Normal)   # H (28 f64), b (7 f64), chi2_photo, chi2_depth (f64), six int32 counts: 320 bytes
JOINT_NORMAL_DTYPE = np.dtype(EllcJointNormal)   # A (8 x 21), a (8 x 6), S (1176), s (48), chi2_photo, chi2_prior (f64), n_terms (i64), six int32 counts and B, n_view_terms (8 int32): 11600 bytes
HYP_FIELDS = ("invDepth", "invDepthSmoothed", "variance", "varianceSmoothed", "validity", "blacklisted", "valid")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_config(width, height, levels=4, **kw):
    cfg = EllcConfig()
    _lib.lib().ellc_default_config(C.byref(cfg), width, height, levels)
    for k, v in kw.items():
        if k == "max_iter":
            mi = list(v) + [12] * (MAX_LEVELS - len(v))
            for i in range(MAX_LEVELS):
                cfg.max_iter[i] = mi[i]
        else:
            setattr(cfg, k, v)
    return cfg


default_diag = False   # tools/diaglib.py sets it: tools create their contexts in the diagnostic library


class Context:
    """Resident keyframe / frame slots, one depth map and an in-order queue of work on the GPU (ellc_ctx); up to three
    alignment batches may be in flight at once (align_enqueue / align_fetch) — 4 x cfg.coalesce with cfg.coalesce > 1, where
    full batches enqueued one after the other run side by side in one launch sequence."""

    def __init__(self, cfg, diag=None):
        """diag=True: the context lives in libellc_hip_diag.so (include/ellc_abi_diag.h: profile_* / selftest_* / debug_* below) — the
        same kernels and launch paths as the shipping library, which does not export those hooks."""
        self.cfg = cfg
        self.diag = default_diag if diag is None else bool(diag)
        self._l = _lib.diag_lib() if self.diag else _lib.lib()
        h = C.c_void_p()
        st = self._l.ellc_ctx_create(C.byref(cfg), C.byref(h))
        self.h = h
        if st != 0:
            msg = self._l.ellc_last_error(h).decode() if h else "context creation failed"
            if h:
                self._l.ellc_ctx_destroy(h)
                self.h = None
            raise EllcError("ellc_ctx_create -> %d: %s" % (st, msg))
        self.levels = cfg.levels

    def close(self):
        if getattr(self, "h", None):
            self._l.ellc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st, what):
        if st != 0:
            raise EllcError("%s -> %d: %s" % (what, st, self._l.ellc_last_error(self.h).decode()))

    def sync(self):
        self._ck(self._l.ellc_sync(self.h), "ellc_sync")

    def counters(self):
        """Diagnostic counters (ELLC_CTR_* of ellc_abi.h): polled / poll_timeout / event_wait / continuation."""
        out = (C.c_longlong * 4)()
        self._ck(self._l.ellc_ctx_counters(self.h, out, 4), "ellc_ctx_counters")
        return dict(polled=out[0], poll_timeout=out[1], event_wait=out[2], continuation=out[3])

    def set_poll_timeout_us(self, us):
        self._ck(self._l.ellc_ctx_set_poll_timeout_us(self.h, int(us)), "ellc_ctx_set_poll_timeout_us")

    def set_grid_batch(self, n):
        """cfg.grid_batch for the calls that follow (ellc_ctx_set_grid_batch)."""
        self._ck(self._l.ellc_ctx_set_grid_batch(self.h, int(n)), "ellc_ctx_set_grid_batch")

    def set_dense_maps(self, mode):
        """0: dense maps take the list-free kernels (default); 1: always the compact lists (ellc_ctx_set_dense_maps)."""
        self._ck(self._l.ellc_ctx_set_dense_maps(self.h, int(mode)), "ellc_ctx_set_dense_maps")

    def set_persistent_schedule(self, mode):
        """1: the state-driven schedule as one resident launch (default); 0: one launch per iteration; 2: test hook, every resident
        launch is abandoned at its first hand-over (ellc_ctx_set_persistent_schedule)."""
        self._ck(self._l.ellc_ctx_set_persistent_schedule(self.h, int(mode)), "ellc_ctx_set_persistent_schedule")

    def level_shape(self, level):
        return (self.cfg.height >> level, self.cfg.width >> level)

    # ---- frame side
    def frame_upload(self, slot, image):
        image = np.ascontiguousarray(image, np.uint8)
        assert image.shape == (self.cfg.height, self.cfg.width)
        self._ck(self._l.ellc_frame_upload(self.h, slot, _p(image)), "ellc_frame_upload")

    def keyframe_upload(self, slot, image):
        image = np.ascontiguousarray(image, np.uint8)
        assert image.shape == (self.cfg.height, self.cfg.width)
        self._ck(self._l.ellc_keyframe_upload(self.h, slot, _p(image)), "ellc_keyframe_upload")

    def keyframe_from_frame(self, kf_slot, frame_slot):
        self._ck(self._l.ellc_keyframe_from_frame(self.h, kf_slot, frame_slot), "ellc_keyframe_from_frame")

    def image_level(self, is_kf, slot, level):
        sw, sh, c, r = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self._l.ellc_get_image_level(self.h, int(is_kf), slot, level, None, C.byref(sw), C.byref(sh), C.byref(c), C.byref(r)),
                 "ellc_get_image_level")
        out = np.zeros((sh.value, sw.value), np.uint8)
        self._ck(self._l.ellc_get_image_level(self.h, int(is_kf), slot, level, _p(out), None, None, None, None), "ellc_get_image_level")
        return out, (r.value, c.value)

    def gradient(self, is_kf, slot, level):
        shp = self.level_shape(level)
        gx = np.zeros(shp, np.float32); gy = np.zeros(shp, np.float32)
        self._ck(self._l.ellc_get_gradient(self.h, int(is_kf), slot, level, _p(gx), _p(gy)), "ellc_get_gradient")
        return gx, gy

    def max_gradient(self, is_kf, slot):
        out = np.zeros((self.cfg.height, self.cfg.width), np.float32)
        n = C.c_int(0)
        self._ck(self._l.ellc_get_max_gradient(self.h, int(is_kf), slot, _p(out), C.byref(n)), "ellc_get_max_gradient")
        return out, n.value

    # ---- keyframe depth / weights
    def keyframe_set_depth(self, slot, depth0, var0):
        d = np.ascontiguousarray(depth0, np.float32); v = np.ascontiguousarray(var0, np.float32)
        self._ck(self._l.ellc_keyframe_set_depth(self.h, slot, _p(d), _p(v)), "ellc_keyframe_set_depth")

    def keyframe_set_depth_level(self, slot, level, depth, var):
        d = np.ascontiguousarray(depth, np.float32); v = np.ascontiguousarray(var, np.float32)
        self._ck(self._l.ellc_keyframe_set_depth_level(self.h, slot, level, _p(d), _p(v)), "ellc_keyframe_set_depth_level")

    def keyframe_depth_level(self, slot, level):
        shp = self.level_shape(level)
        d = np.zeros(shp, np.float32); v = np.zeros(shp, np.float32)
        self._ck(self._l.ellc_keyframe_get_depth_level(self.h, slot, level, _p(d), _p(v)), "ellc_keyframe_get_depth_level")
        return d, v

    def keyframe_set_weights(self, slot, level, w, num_added=1):
        w = np.ascontiguousarray(w, np.float32)
        self._ck(self._l.ellc_keyframe_set_weights(self.h, slot, level, _p(w), num_added), "ellc_keyframe_set_weights")

    def keyframe_weights(self, slot, level):
        w = np.zeros(self.level_shape(level), np.float32)
        n = C.c_int(0)
        self._ck(self._l.ellc_keyframe_get_weights(self.h, slot, level, _p(w), C.byref(n)), "ellc_keyframe_get_weights")
        return w, n.value

    def keyframe_finalise_weights(self, slot):
        self._ck(self._l.ellc_keyframe_finalise_weights(self.h, slot), "ellc_keyframe_finalise_weights")

    # ---- alignment
    def _batch(self, kf_slots, frame_slots, init_pose):
        kf = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        fr = np.ascontiguousarray(frame_slots, np.int32).reshape(-1)
        B = kf.size
        assert fr.size == B
        ip = np.zeros((B, 6), np.float32) if init_pose is None else np.ascontiguousarray(init_pose, np.float32).reshape(B, 6)
        return B, kf, fr, ip

    def align(self, kf_slots, frame_slots, init_pose=None, mode=MODE_FCA, save_weights=False):
        B, kf, fr, ip = self._batch(kf_slots, frame_slots, init_pose)
        pose = np.zeros((B, 6), np.float32); iters = np.zeros((B, self.levels), np.int32); wgt = np.zeros(B, np.float32)
        self._ck(self._l.ellc_align(self.h, B, _p(kf), _p(fr), _p(ip), mode, int(save_weights), _p(pose), _p(iters), _p(wgt)), "ellc_align")
        return pose, iters, wgt

    def align_enqueue(self, kf_slots, frame_slots, init_pose=None, mode=MODE_FCA, save_weights=False):
        B, kf, fr, ip = self._batch(kf_slots, frame_slots, init_pose)
        self._ck(self._l.ellc_align_enqueue(self.h, B, _p(kf), _p(fr), _p(ip), mode, int(save_weights)), "ellc_align_enqueue")
        return B

    def align_fetch(self, B):
        pose = np.zeros((B, 6), np.float32); iters = np.zeros((B, self.levels), np.int32); wgt = np.zeros(B, np.float32)
        self._ck(self._l.ellc_align_fetch(self.h, B, _p(pose), _p(iters), _p(wgt)), "ellc_align_fetch")
        return pose, iters, wgt

    def align_quality(self, kf_slots, frame_slots, pose, level=0):
        """ellc_align_quality_at: one forward-compositional pixel pass per (keyframe slot, frame slot, pose) at `level`, no update.
        Returns a dict of arrays over the B evaluations: n_depth, n_used (int32), sum_r2, sum_abs_r, sum_w, sum_wr2 (f64), H [B][6][6],
        b [B][6], Hinv [B][6][6] (f32), and the derived rms = sqrt(sum_r2 / n_used), wrms = sqrt(sum_wr2 / sum_w),
        overlap = n_used / n_depth (0 where the denominator is 0)."""
        B, kf, fr, ps = self._batch(kf_slots, frame_slots, pose)
        rec = (EllcAlignQuality * B)()
        self._ck(self._l.ellc_align_quality_at(self.h, B, _p(kf), _p(fr), _p(ps), int(level), rec), "ellc_align_quality_at")
        raw = np.frombuffer(rec, dtype=np.dtype(EllcAlignQuality)).copy()
        out = {k: raw[k].copy() for k in ("n_depth", "n_used", "sum_r2", "sum_abs_r", "sum_w", "sum_wr2")}
        out["H"] = raw["H"].reshape(B, 6, 6).copy()
        out["b"] = raw["b"].reshape(B, 6).copy()
        out["Hinv"] = raw["Hinv"].reshape(B, 6, 6).copy()

        def ratio(num, den):
            den = np.asarray(den, np.float64)
            return np.divide(np.asarray(num, np.float64), den, out=np.zeros(B, np.float64), where=den != 0)
        out["rms"] = np.sqrt(ratio(out["sum_r2"], out["n_used"]))
        out["wrms"] = np.sqrt(ratio(out["sum_wr2"], out["sum_w"]))
        out["overlap"] = ratio(out["n_used"], out["n_depth"])
        return out

    def gn_iterate(self, kf_slot, frame_slot, level, pose, mode=MODE_FCA, it=0, planes=False):
        pose = np.ascontiguousarray(pose, np.float32)
        H = np.zeros((6, 6), np.float32); b = np.zeros(6, np.float32); d = np.zeros(6, np.float32); p = np.zeros(6, np.float32)
        w = C.c_float(0)
        shp = self.level_shape(level)
        pl = np.zeros((10,) + shp, np.float32) if planes else None
        self._ck(self._l.ellc_gn_iterate(self.h, kf_slot, frame_slot, level, mode, it, _p(pose), _p(H), _p(b), _p(d), _p(p), C.byref(w), _p(pl)),
                 "ellc_gn_iterate")
        out = dict(H=H, b=b, delta=d, pose=p, weighted=w.value)
        if planes:
            out.update(residual=pl[0], weight=pl[1], warpedX=pl[2], warpedY=pl[3], J=pl[4:10])
        return out

    def gn_display_planes(self, kf_slot, frame_slot, level, pose):
        """display_templateimg / display_2bewarpedimg (u8), display_warpedimg / display_origres (f32) of one pass."""
        pose = np.ascontiguousarray(pose, np.float32)
        shp = self.level_shape(level)
        t = np.zeros(shp, np.uint8); k = np.zeros(shp, np.uint8); w = np.zeros(shp, np.float32); o = np.zeros(shp, np.float32)
        self._ck(self._l.ellc_gn_display_planes(self.h, kf_slot, frame_slot, level, _p(pose), _p(t), _p(k), _p(w), _p(o)), "ellc_gn_display_planes")
        return dict(templateimg=t, tobewarpedimg=k, warpedimg=w, origres=o)

    # ---- depth map
    def _hyp(self, st):
        arrs = [np.ascontiguousarray(st["invDepth"], np.float32), np.ascontiguousarray(st["invDepthSmoothed"], np.float32),
                np.ascontiguousarray(st["variance"], np.float32), np.ascontiguousarray(st["varianceSmoothed"], np.float32),
                np.ascontiguousarray(st["validity"], np.int32), np.ascontiguousarray(st["blacklisted"], np.int32),
                np.ascontiguousarray(st["valid"], np.uint8)]
        h = EllcHypotheses(*[a.ctypes.data for a in arrs])
        return h, arrs

    def depth_set_state(self, st):
        h, keep = self._hyp(st)
        self._ck(self._l.ellc_depth_set_state(self.h, C.byref(h)), "ellc_depth_set_state")

    def depth_get_state(self):
        shp = (self.cfg.height, self.cfg.width)
        st = dict(invDepth=np.zeros(shp, np.float32), invDepthSmoothed=np.zeros(shp, np.float32), variance=np.zeros(shp, np.float32),
                  varianceSmoothed=np.zeros(shp, np.float32), validity=np.zeros(shp, np.int32), blacklisted=np.zeros(shp, np.int32),
                  valid=np.zeros(shp, np.uint8))
        h, keep = self._hyp(st)
        self._ck(self._l.ellc_depth_get_state(self.h, C.byref(h)), "ellc_depth_get_state")
        return dict(zip(HYP_FIELDS, keep))

    def depth_set_keyframe(self, slot):
        self._ck(self._l.ellc_depth_set_keyframe(self.h, slot), "ellc_depth_set_keyframe")

    def depth_propagate(self, new_kf_slot, pose_new_wrt_old):
        p = np.ascontiguousarray(pose_new_wrt_old, np.float32)
        self._ck(self._l.ellc_depth_propagate(self.h, new_kf_slot, _p(p)), "ellc_depth_propagate")

    def depth_observe(self, frame_slot, pose_frame_wrt_kf):
        p = np.ascontiguousarray(pose_frame_wrt_kf, np.float32)
        self._ck(self._l.ellc_depth_observe(self.h, frame_slot, _p(p)), "ellc_depth_observe")

    def depth_fill_holes(self):
        self._ck(self._l.ellc_depth_fill_holes(self.h), "ellc_depth_fill_holes")

    def depth_regularize(self, remove_occlusions=False):
        self._ck(self._l.ellc_depth_regularize(self.h, int(remove_occlusions)), "ellc_depth_regularize")

    def depth_do_regularization(self, remove_occlusions=False):
        """doRegularization (:1627-1635): fill holes + regularise in one launch."""
        self._ck(self._l.ellc_depth_do_regularization(self.h, int(remove_occlusions)), "ellc_depth_do_regularization")

    def depth_regularize_fill_regularize(self, remove_occlusions=True):
        """regularise(remove_occlusions) + fill holes + regularise(False) in one launch (createKeyFrame's middle)"""
        self._ck(self._l.ellc_depth_regularize_fill_regularize(self.h, int(remove_occlusions)), "ellc_depth_regularize_fill_regularize")

    def depth_make_inv_depth_one(self):
        f = C.c_float(0)
        self._ck(self._l.ellc_depth_make_inv_depth_one(self.h, C.byref(f)), "ellc_depth_make_inv_depth_one")
        return f.value

    def depth_update_depth_image(self):
        self._ck(self._l.ellc_depth_update_depth_image(self.h), "ellc_depth_update_depth_image")

    def depth_create_keyframe(self, new_kf_slot, pose_new_wrt_old):
        p = np.ascontiguousarray(pose_new_wrt_old, np.float32)
        f = C.c_float(0)
        self._ck(self._l.ellc_depth_create_keyframe(self.h, new_kf_slot, _p(p), C.byref(f)), "ellc_depth_create_keyframe")
        return f.value

    def track_frame(self, frame_slot, init_pose=None, save_weights=False):
        """ellc_track_frame: alignment against the depth map's keyframe + observe / fill holes / regularise / export behind it on the
        device. Returns pose (6,), iters (levels,), weightedPose, seeds percent (of the map before the observation)."""
        ip = np.zeros(6, np.float32) if init_pose is None else np.ascontiguousarray(init_pose, np.float32).reshape(6)
        pose = np.zeros(6, np.float32); iters = np.zeros(self.levels, np.int32); w = C.c_float(0); sd = C.c_float(0)
        self._ck(self._l.ellc_track_frame(self.h, frame_slot, _p(ip), int(save_weights), _p(pose), _p(iters), C.byref(w), C.byref(sd)), "ellc_track_frame")
        return pose, iters, w.value, sd.value

    def depth_seeds(self):
        f = C.c_float(0)
        self._ck(self._l.ellc_depth_seeds(self.h, C.byref(f)), "ellc_depth_seeds")
        return f.value

    # ---- frame ingest (Frame.cpp:45-75 after the decode)
    def ingest_configure(self, orig_w, orig_h, fx, fy, cx, cy, dist5=None, do_undistort=True):
        d = np.ascontiguousarray(dist5 if dist5 is not None else np.zeros(5), np.float32)
        kn = np.zeros(4, np.float32)
        self._ck(self._l.ellc_ingest_configure(self.h, int(orig_w), int(orig_h), C.c_float(fx), C.c_float(fy), C.c_float(cx), C.c_float(cy),
                                               _p(d), int(bool(do_undistort)), _p(kn)), "ellc_ingest_configure")
        return kn

    def frame_ingest_bgr(self, slot, bgr, probes=False):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        W, H = self.cfg.width, self.cfg.height
        if probes:
            g = np.zeros((H, W), np.uint8); u = np.zeros((H, W, 4), np.uint8)
            self._ck(self._l.ellc_frame_ingest_bgr(self.h, slot, _p(bgr), _p(g), _p(u)), "ellc_frame_ingest_bgr")
            return g, u
        self._ck(self._l.ellc_frame_ingest_bgr(self.h, slot, _p(bgr), None, None), "ellc_frame_ingest_bgr")

    # ---- loop-closure support
    def histogram(self, is_kf, slot):
        h = np.zeros(256, np.float32)
        self._ck(self._l.ellc_histogram(self.h, int(is_kf), slot, _p(h)), "ellc_histogram")
        return h

    def copy_slot(self, dst_is_kf, dst, src_is_kf, src):
        self._ck(self._l.ellc_copy_slot(self.h, int(dst_is_kf), dst, int(src_is_kf), src), "ellc_copy_slot")

    # ---- the map as points
    def map_points_raw(self, kf_slots, T12, out, capacity, level=0, max_var=0.0, min_support=0, support_k2=1.0, stride=1):
        """ellc_keyframe_map_points with the caller's buffer: `out` is None (the sizing call) or a writable array of at least
        capacity * 24 bytes. Returns (status, counts, total) — the status is NOT raised, so that ELLC_ERR_CAPACITY can be looked at."""
        kf = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        B = kf.size
        T = np.ascontiguousarray(T12, np.float32).reshape(B, 12)
        flt = EllcMapFilter(max_var, int(min_support), support_k2, int(stride))
        counts = np.zeros(B, np.int32)
        total = C.c_int(0)
        st = self._l.ellc_keyframe_map_points(self.h, B, _p(kf), _p(T), int(level), C.byref(flt), _p(out), int(capacity), _p(counts), C.byref(total))
        return st, counts, total.value

    def map_points(self, kf_slots, T12, level=0, max_var=0.0, min_support=0, support_k2=1.0, stride=1):
        """The keyframe slots' semi-dense maps on `level` as filtered 3-D points (ellc_keyframe_map_points): T12[b] is the row-major
        3x4 transform of request b. Returns (points, counts): a structured array of MAP_POINT_DTYPE in request-major raster order and
        the points per request."""
        kw = dict(level=level, max_var=max_var, min_support=min_support, support_k2=support_k2, stride=stride)
        st, counts, total = self.map_points_raw(kf_slots, T12, None, 0, **kw)
        self._ck(st, "ellc_keyframe_map_points")
        pts = np.zeros(total, MAP_POINT_DTYPE)
        st, counts, total = self.map_points_raw(kf_slots, T12, pts, total, **kw)
        self._ck(st, "ellc_keyframe_map_points")
        return pts, counts

    # ---- the map rendered into a view
    def _render(self, fn, name, extra, kf_slots, T12, level, agree_k2, dst_slot, max_var, min_support, support_k2, stride, out=None):
        kf = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        B = kf.size
        T = np.ascontiguousarray(T12, np.float32).reshape(B, 12)
        flt = EllcMapFilter(max_var, int(min_support), support_k2, int(stride))
        shp = self.level_shape(level) if 0 <= level < self.levels else (1, 1)   # (a level out of range is the library's to refuse)
        if out is None:
            out = dict(depth=np.zeros(shp, np.float32), var=np.zeros(shp, np.float32), source=np.zeros(shp, np.int32),
                       agree=np.zeros(shp, np.int32), intensity=np.zeros(shp, np.uint8))
        for k, dt in (("depth", np.float32), ("var", np.float32), ("source", np.int32), ("agree", np.int32), ("intensity", np.uint8)):
            assert out[k].dtype == dt and out[k].shape == shp and out[k].flags.c_contiguous, k
        n = C.c_int(0)
        self._ck(fn(self.h, B, _p(kf), _p(T), int(level), C.byref(flt), C.c_float(agree_k2), int(dst_slot), _p(out["depth"]), _p(out["var"]),
                    _p(out["source"]), _p(out["agree"]), _p(out["intensity"]), C.byref(n), *extra), name)
        out["n_valid"] = n.value
        return out

    def render_depth(self, kf_slots, T12, level=0, agree_k2=1.0, dst_slot=-1, max_var=0.0, min_support=0, support_k2=1.0, stride=1, out=None):
        """The keyframe slots' maps on `level` splatted into one view (ellc_keyframe_render_depth): T12[b] is the row-major 3x4 transform
        from keyframe b's camera into the view's. Returns a dict of the planes depth, var (f32), source, agree (int32), intensity
        (uint8), each (rows, cols) of the level, and n_valid. dst_slot >= 0 (level 0 only) also leaves depth / var in that keyframe
        slot, as keyframe_set_depth would. out: a dict of such planes from an earlier call, written again instead of new arrays."""
        return self._render(self._l.ellc_keyframe_render_depth, "ellc_keyframe_render_depth", (), kf_slots, T12, level, agree_k2, dst_slot,
                            max_var, min_support, support_k2, stride, out)

    # ---- the maps fused in a view
    def _fuse(self, fn, name, extra, kf_slots, T12, level, agree_k2, max_merge, dst_slot, max_var, min_support, support_k2, stride, out=None):
        kf = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        B = kf.size
        T = np.ascontiguousarray(T12, np.float32).reshape(B, 12)
        flt = EllcMapFilter(max_var, int(min_support), support_k2, int(stride))
        shp = self.level_shape(level) if 0 <= level < self.levels else (1, 1)   # (a level out of range is the library's to refuse)
        kinds = (("depth", np.float32), ("var", np.float32), ("source", np.int32), ("agree", np.int32), ("merged", np.int32), ("intensity", np.uint8))
        if out is None:
            out = {k: np.zeros(shp, dt) for k, dt in kinds}
        for k, dt in kinds:
            assert out[k].dtype == dt and out[k].shape == shp and out[k].flags.c_contiguous, k
        n = C.c_int(0); nf = C.c_int(0)
        self._ck(fn(self.h, B, _p(kf), _p(T), int(level), C.byref(flt), C.c_float(agree_k2), int(max_merge), int(dst_slot), _p(out["depth"]),
                    _p(out["var"]), _p(out["source"]), _p(out["agree"]), _p(out["merged"]), _p(out["intensity"]), C.byref(n), C.byref(nf), *extra), name)
        out["n_valid"] = n.value
        out["n_fused"] = nf.value
        return out

    def fuse_depth(self, kf_slots, T12, level=0, agree_k2=1.0, max_merge=64, dst_slot=-1, max_var=0.0, min_support=0, support_k2=1.0, stride=1,
                   out=None):
        """render_depth with the candidates that agree with a target's winner merged into it in ascending (request, raster index) order,
        at most max_merge per target (ellc_keyframe_fuse_depth). Returns render_depth's dict with the plane merged (int32: hypotheses
        fused into the target, the winner included) and n_fused (targets with merged >= 2) added; source, agree, intensity and n_valid
        are the render's. dst_slot >= 0 (level 0 only) also leaves depth / var in that keyframe slot, which may be one of kf_slots."""
        return self._fuse(self._l.ellc_keyframe_fuse_depth, "ellc_keyframe_fuse_depth", (), kf_slots, T12, level, agree_k2, max_merge, dst_slot,
                          max_var, min_support, support_k2, stride, out)

    # ---- keyframe maps folded into the live depth map
    def _absorb(self, fn, name, extra, kf_slots, T12, params, max_var, min_support, support_k2, stride, stats, tail=None, lights=None, head=()):
        kf = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        B = kf.size
        T = np.ascontiguousarray(T12, np.float32).reshape(B, 12)
        light = ()
        if lights is not None:   # the _lit entry point of the same call: the lights go behind the transforms
            fn, name = getattr(self._l, name + "_lit"), name + "_lit"
            L = np.ascontiguousarray(lights, np.float32).reshape(B, 2)
            light = (_p(L),)
        flt = EllcMapFilter(max_var, int(min_support), support_k2, int(stride))
        prm = params if isinstance(params, EllcAbsorbParams) else absorb_params(**(params or {}))
        st = stats if stats is not None else EllcAbsorbStats()
        # (head: arguments in front of B - the restart's new keyframe slot; tail: in front of the stats pointer - its rescale factor)
        self._ck(fn(self.h, *head, B, _p(kf), _p(T), *light, C.byref(flt), C.byref(prm), *(tail or ()), C.byref(st), *extra), name)
        return {k: int(getattr(st, k)) for k in ABSORB_STATS_FIELDS}

    def depth_absorb(self, kf_slots, T12, params=None, max_var=0.0, min_support=0, support_k2=1.0, stride=1, stats=None, lights=None):
        """The maps of keyframe slots kf_slots[b] (level 0) folded into the context's live depth map (ellc_depth_absorb_keyframes):
        T12[b] is the row-major 3x4 transform from that slot's camera into the depth map's keyframe's, the filter is map_points'.
        params: dict of agree_k2, max_fold, photo_gate, src_validity, finalise (defaults 1, 64, 1, 20, 1) or an EllcAbsorbParams.
        Returns the sixteen counts of ellc_absorb_stats as a dict (stats: an EllcAbsorbStats to receive them as well). With
        finalise=0 the caller must regularise (depth_do_regularization) before anything observes or exports the map.
        lights: [B][2] f32 (gain, offset) taking slot kf_slots[b]'s grey values into the keyframe's, the direction of T12[b]; the
        photometric gate's residual is then taken against gain * Is + offset (ellc_depth_absorb_keyframes_lit). None: the unlit call."""
        return self._absorb(self._l.ellc_depth_absorb_keyframes, "ellc_depth_absorb_keyframes", (), kf_slots, T12, params, max_var, min_support,
                            support_k2, stride, stats, lights=lights)

    def depth_restart(self, new_kf_slot, kf_slots, T12, params=None, max_var=0.0, min_support=0, support_k2=1.0, stride=1, stats=None, lights=None):
        """The live depth map re-seated on keyframe slot new_kf_slot (which holds an image and is not among kf_slots) from the maps of
        keyframe slots kf_slots[b], starting EMPTY (ellc_depth_restart_from_keyframes): the wipe, depth_absorb's fold with T12[b] the
        transform from slot kf_slots[b]'s camera into new_kf_slot's, and with finalise=1 (the default) createKeyFrame's tail. The
        context needs no state beforehand. Returns (the sixteen counts of ellc_absorb_stats as a dict, the rescale factor).
        lights: as in depth_absorb, into new_kf_slot's grey values (ellc_depth_restart_from_keyframes_lit); None: the unlit call."""
        factor = C.c_float(0.0)
        out = self._absorb(self._l.ellc_depth_restart_from_keyframes, "ellc_depth_restart_from_keyframes", (), kf_slots, T12, params, max_var,
                           min_support, support_k2, stride, stats, tail=(C.byref(factor),), lights=lights, head=(int(new_kf_slot),))
        return out, float(factor.value)

    # ---- trial propagation: what a keyframe's map would seed in an image
    def _trial(self, fn, name, extra, src_slots, dst_slots, Ts, dst_is_keyframe, photo_gate, max_var, min_support, support_k2, stride):
        src = np.ascontiguousarray(src_slots, np.int32).reshape(-1)
        dst = np.ascontiguousarray(dst_slots, np.int32).reshape(-1)
        B = src.size
        assert dst.size == B
        T = np.ascontiguousarray(Ts, np.float32).reshape(B, 12)
        flt = EllcMapFilter(max_var, int(min_support), support_k2, int(stride))
        out = np.zeros(B, np.dtype(EllcTrialPropagation))
        self._ck(fn(self.h, B, _p(src), int(dst_is_keyframe), _p(dst), _p(T), C.byref(flt), int(photo_gate), _p(out), *extra), name)
        return out

    def trial_propagate(self, src_slots, dst_slots, Ts, dst_is_keyframe=False, photo_gate=1, max_var=0.0, min_support=0, support_k2=1.0, stride=1):
        """What propagating keyframe slot src_slots[b]'s map into the image of slot dst_slots[b] (a frame slot, or a keyframe slot with
        dst_is_keyframe) at Ts[b] (row-major 3x4, source camera into destination camera) would give (ellc_keyframe_trial_propagate): a
        structured array of B ellc_trial_propagation records - n_kept, n_in_view, n_interior, n_low_grad, n_candidates, n_targets
        (int32), sum_r2, sum_abs_r (f64). n_targets is the number of hypotheses a restart from that request alone would create."""
        return self._trial(self._l.ellc_keyframe_trial_propagate, "ellc_keyframe_trial_propagate", (), src_slots, dst_slots, Ts, dst_is_keyframe,
                           photo_gate, max_var, min_support, support_k2, stride)

    def trial_propagate_lit(self, src_slots, dst_slots, Ts, lights=None, dst_is_keyframe=False, photo_gate=1, max_var=0.0, min_support=0,
                            support_k2=1.0, stride=1):
        """trial_propagate with the residual taken against gain * Is + offset at lights[b] ([B][2] f32, source's grey values into the
        destination's; None: (1, 0) each) (ellc_keyframe_trial_propagate_lit): a structured array of B ellc_trial_propagation_lit
        records (TRIAL_LIT_DTYPE) - trial_propagate's fields at that light, then sum_s, sum_t, sum_ss, sum_st, sum_tt (f64) and n_fit
        over the interior pixels, which trial_light_solve turns into a light."""
        src = np.ascontiguousarray(src_slots, np.int32).reshape(-1)
        dst = np.ascontiguousarray(dst_slots, np.int32).reshape(-1)
        B = src.size
        assert dst.size == B
        T = np.ascontiguousarray(Ts, np.float32).reshape(B, 12)
        L = None if lights is None else np.ascontiguousarray(lights, np.float32).reshape(B, 2)
        flt = EllcMapFilter(max_var, int(min_support), support_k2, int(stride))
        out = np.zeros(B, TRIAL_LIT_DTYPE)
        self._ck(self._l.ellc_keyframe_trial_propagate_lit(self.h, B, _p(src), int(dst_is_keyframe), _p(dst), _p(T), _p(L), C.byref(flt),
                                                           int(photo_gate), _p(out)), "ellc_keyframe_trial_propagate_lit")
        return out

    # ---- one keyframe's map against another's
    def _consistency(self, fn, name, extra, src_slots, dst_slots, Ts, level, agree_k2, max_var, min_support, support_k2, stride):
        src = np.ascontiguousarray(src_slots, np.int32).reshape(-1)
        dst = np.ascontiguousarray(dst_slots, np.int32).reshape(-1)
        B = src.size
        assert dst.size == B
        T = np.ascontiguousarray(Ts, np.float32).reshape(B, 12)
        flt = EllcMapFilter(max_var, int(min_support), support_k2, int(stride))
        out = np.zeros(B, np.dtype(EllcDepthConsistency))
        self._ck(fn(self.h, B, _p(src), _p(dst), _p(T), int(level), C.byref(flt), C.c_float(agree_k2), _p(out), *extra), name)
        return out

    def depth_consistency(self, src_slots, dst_slots, Ts, level=0, agree_k2=1.0, max_var=0.0, min_support=0, support_k2=1.0, stride=1):
        """Keyframe slot src_slots[b]'s map on `level` against slot dst_slots[b]'s (ellc_keyframe_depth_consistency): Ts[b] is the
        row-major 3x4 transform from the source's camera into the destination's. Returns a structured array of B
        ellc_depth_consistency records: n_kept, n_in_view, n_overlap, n_agree, n_in_front, n_behind, n_weighted (int32), sum_abs_di,
        sum_di2 (int64), sum_chi2, sum_w_ss, sum_w_st (f64); sum_w_st / sum_w_ss is the scale that takes the source's inverse depths
        onto the destination's."""
        return self._consistency(self._l.ellc_keyframe_depth_consistency, "ellc_keyframe_depth_consistency", (), src_slots, dst_slots, Ts, level,
                                 agree_k2, max_var, min_support, support_k2, stride)

    # ---- Sim(3) refinement of a pair of keyframes
    def _sim3_args(self, src_slots, dst_slots, Ts, max_var, min_support, support_k2, stride, params):
        src = np.ascontiguousarray(src_slots, np.int32).reshape(-1)
        dst = np.ascontiguousarray(dst_slots, np.int32).reshape(-1)
        B = src.size
        assert dst.size == B
        T = np.ascontiguousarray(Ts, np.float32).reshape(B, 12)
        return B, src, dst, T, EllcMapFilter(max_var, int(min_support), support_k2, int(stride)), sim3_params(**(params or {}))

    def sim3_step(self, src_slots, dst_slots, Ts, level=0, max_var=0.0, min_support=0, support_k2=1.0, stride=1, params=None):
        """The normal equations of one seven-parameter Gauss-Newton step (ellc_keyframe_sim3_step) of keyframe slot src_slots[b] against
        slot dst_slots[b] on `level` at Ts[b], the row-major 3x4 transform from the source's camera into the destination's with the scale
        in its 3x3 block. params: dict of sigma_i2, huber_k, gate_k2, depth_weight (defaults 16, 1.345, 9, 1). Returns a structured
        array of B ellc_sim3_normal records: H (28, upper triangle by rows), b (7), chi2_photo, chi2_depth (f64), n_kept, n_in_view,
        n_photo, n_photo_huber, n_depth, n_depth_gated (int32). A step solves H xi = -b (sim3_solve) and T <- sim3_apply(xi, T)."""
        return self._pair_step("ellc_keyframe_sim3_step", SIM3_NORMAL_DTYPE, (), src_slots, dst_slots, Ts, level, max_var, min_support, support_k2, stride,
                               params)

    def _pair_step(self, name, dtype, lights, src_slots, dst_slots, Ts, level=0, max_var=0.0, min_support=0, support_k2=1.0, stride=1, params=None, tail=()):
        """The pair steps that return one record a pair (sim3_step, light_step, sim3_step_lit and their ellc_profile_* twins): entry
        point `name`, records of `dtype`; lights is () for the call that takes no light, (lights,) for the others; tail follows `out`."""
        B, src, dst, T, flt, prm = self._sim3_args(src_slots, dst_slots, Ts, max_var, min_support, support_k2, stride, params)
        li = [self._lights(l, B) for l in lights]
        out = np.zeros(B, dtype)
        self._ck(getattr(self._l, name)(self.h, B, _p(src), _p(dst), _p(T), *[_p(l) for l in li], int(level), C.byref(flt), C.byref(prm), _p(out), *tail),
                 name)
        return out

    def _align(self, name, lit, src_slots, dst_slots, Ts, lights, level_from, level_to, max_iter, eps, max_var, min_support, support_k2, stride, params,
               light_params, trace):
        """sim3_align (lit false: no light, no light parameters, no light outputs or traces) and sim3_align_lit: the outputs, the
        traces, the call, and each pair's traces cut to the evaluations it had (n_kept >= 0 in its trace_rec)."""
        B, src, dst, T, flt, prm = self._sim3_args(src_slots, dst_slots, Ts, max_var, min_support, support_k2, stride, params)
        n_levels = max(int(level_from) - int(level_to) + 1, 1)
        cap = n_levels * max(int(max_iter), 1) + 1
        res = dict(T=np.zeros((B, 12), np.float32), rec=np.zeros(B, SIM3_NORMAL_DTYPE), iters=np.zeros((B, n_levels), np.int32))
        tr = dict(trace_T=np.zeros((B, cap, 12), np.float32), trace_rec=np.zeros((B, cap), SIM3_NORMAL_DTYPE)) if trace else {}
        fixed = (int(level_from), int(level_to), C.byref(flt), C.byref(prm))
        if lit:
            li = self._lights(lights, B)
            lp = _as_light_params(light_params)
            res.update(light=np.zeros((B, 2), np.float32), light_rec=np.zeros(B, LIGHT_NORMAL_DTYPE))
            if trace:
                tr.update(trace_light=np.zeros((B, cap, 2), np.float32), trace_light_rec=np.zeros((B, cap), LIGHT_NORMAL_DTYPE))
            args = (_p(li),) + fixed + (C.byref(lp), int(max_iter), C.c_float(eps), _p(res["T"]), _p(res["light"]), _p(res["rec"]), _p(res["light_rec"]),
                                        _p(res["iters"]), _p(tr.get("trace_T")), _p(tr.get("trace_rec")), _p(tr.get("trace_light")), _p(tr.get("trace_light_rec")))
        else:
            args = fixed + (int(max_iter), C.c_float(eps), _p(res["T"]), _p(res["rec"]), _p(res["iters"]), _p(tr.get("trace_T")), _p(tr.get("trace_rec")))
        self._ck(getattr(self._l, name)(self.h, B, _p(src), _p(dst), _p(T), *args, cap if trace else 0), name)
        if trace:
            n = [int((tr["trace_rec"][b]["n_kept"] >= 0).sum()) for b in range(B)]
            res.update({k: [t[b, :n[b]].copy() for b in range(B)] for k, t in tr.items()})
        return res

    def sim3_align(self, src_slots, dst_slots, Ts, level_from=0, level_to=0, max_iter=10, eps=1e-4, max_var=0.0, min_support=0, support_k2=1.0,
                   stride=1, params=None, trace=False):
        """The Gauss-Newton loop over sim3_step (ellc_keyframe_sim3_align), coarse to fine from level_from down to level_to, at most
        max_iter updates per level, a pair leaving a level when max |xi_i| <= eps or its system is singular. Returns dict(T = [B][12]
        f32, rec = the records at those T, iters = [B][levels visited] updates per level) and, with trace=True, trace_T / trace_rec:
        per pair the T of every evaluation in order and its record (the final evaluation included)."""
        return self._align("ellc_keyframe_sim3_align", False, src_slots, dst_slots, Ts, None, level_from, level_to, max_iter, eps, max_var, min_support,
                           support_k2, stride, params, None, trace)

    # ---- affine brightness in the Sim(3) refinement: Ip = gain * Is + offset, a light is (gain, offset) per pair, None means (1, 0)
    @staticmethod
    def _lights(lights, B):
        return None if lights is None else np.ascontiguousarray(lights, np.float32).reshape(B, 2)

    def light_step(self, src_slots, dst_slots, Ts, lights=None, level=0, max_var=0.0, min_support=0, support_k2=1.0, stride=1, params=None):
        """The normal equations of the weighted fit of Iw on Is (ellc_keyframe_light_step) over the photometric pixels of sim3_step at
        Ts[b], the Huber weights taken at lights[b]. params: as sim3_step (sigma_i2 and huber_k are read). Returns a structured array
        of B ellc_light_normal records: sum_w, sum_w_s, sum_w_t, sum_w_ss, sum_w_st, sum_w_tt, chi2_photo (f64), n_kept, n_in_view,
        n_photo, n_photo_huber (int32). light_solve turns a record into a light."""
        return self._pair_step("ellc_keyframe_light_step", LIGHT_NORMAL_DTYPE, (lights,), src_slots, dst_slots, Ts, level, max_var, min_support, support_k2,
                               stride, params)

    def sim3_step_lit(self, src_slots, dst_slots, Ts, lights=None, level=0, max_var=0.0, min_support=0, support_k2=1.0, stride=1, params=None):
        """sim3_step with the photometric residual taken against gain * Is + offset (ellc_keyframe_sim3_step_lit); lights None, or (1, 0)
        for a pair, gives sim3_step's bytes."""
        return self._pair_step("ellc_keyframe_sim3_step_lit", SIM3_NORMAL_DTYPE, (lights,), src_slots, dst_slots, Ts, level, max_var, min_support,
                               support_k2, stride, params)

    def sim3_align_lit(self, src_slots, dst_slots, Ts, lights=None, level_from=0, level_to=0, max_iter=10, eps=1e-4, max_var=0.0, min_support=0,
                       support_k2=1.0, stride=1, params=None, light_params=None, trace=False):
        """sim3_align's loop with the light fitted before every Gauss-Newton step (ellc_keyframe_sim3_align_lit): per evaluation the
        light record at (T, l), l' = light_solve of it, the Sim(3) record at (T, l'). light_params: dict of gain_min, gain_max,
        min_pixels (defaults 0.25, 4, 16). Returns dict(T, light = [B][2] f32, rec, light_rec, iters) and, with trace=True, trace_T,
        trace_light, trace_rec, trace_light_rec per pair in order of evaluation (the final evaluation included)."""
        return self._align("ellc_keyframe_sim3_align_lit", True, src_slots, dst_slots, Ts, lights, level_from, level_to, max_iter, eps, max_var,
                           min_support, support_k2, stride, params, light_params, trace)

    # ---- one keyframe slot against B views: what refine_depth, sweep_depth, cull_depth and the joint calls make of their arguments
    def _views_args(self, view_slots, Ts, lights, level, flt=None):
        """(B, view slots, [B][12] transforms, lights or None, (rows, cols) of the level) and, with flt = (max_var, min_support,
        support_k2, stride), the ellc_map_filter behind them."""
        vs = np.ascontiguousarray(view_slots, np.int32).reshape(-1)
        B = vs.size
        out = (B, vs, np.ascontiguousarray(Ts, np.float32).reshape(B, 12), self._lights(lights, B), self.level_shape(level))
        return out if flt is None else out + (EllcMapFilter(flt[0], int(flt[1]), flt[2], int(flt[3])),)

    # ---- a keyframe's map refined against other views
    def _refine(self, name, tail, kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, max_var, min_support, support_k2, stride, params):
        B, vs, T, li, (rows, cols), flt = self._views_args(view_slots, Ts, lights, level, (max_var, min_support, support_k2, stride))
        prm = params if isinstance(params, EllcRefineParams) else refine_default_params(**(params or {}))
        res = dict(depth=np.zeros((rows, cols), np.float32), var=np.zeros((rows, cols), np.float32), views=np.zeros((rows, cols), np.uint8),
                   status=np.zeros((rows, cols), np.uint8))
        st = EllcRefineStats()
        self._ck(getattr(self._l, name)(self.h, int(kf_slot), int(level), B, int(views_are_keyframes), _p(vs), _p(T), _p(li), C.byref(flt), C.byref(prm),
                                        int(dst_slot), _p(res["depth"]), _p(res["var"]), _p(res["views"]), _p(res["status"]), C.byref(st), *tail), name)
        res["stats"] = {f[0]: (list(getattr(st, f[0])) if f[0] == "reserved" else getattr(st, f[0])) for f in EllcRefineStats._fields_}
        return res

    def refine_depth(self, kf_slot, view_slots, Ts, lights=None, level=0, views_are_keyframes=True, dst_slot=-1, max_var=0.0, min_support=0,
                     support_k2=1.0, stride=1, params=None):
        """The per-pixel photometric Gauss-Newton on the inverse depths of keyframe slot kf_slot against the images of the views
        (ellc_keyframe_refine_depth): view b is slot view_slots[b] (keyframe slots, or frame slots with views_are_keyframes=False), Ts[b]
        the row-major 3x4 transform from the keyframe's camera into the view's, lights[b] its (gain, offset) with the keyframe as the
        source (None: (1, 0)). params: an ellc_refine_params (refine_default_params()) or a dict of sigma_i2, huber_k, prior_weight,
        max_step_rel, n_iter, min_views (defaults 16, 1.345, 1, 0.5, 3, 2). dst_slot >= 0 (level 0 only) stores the planes into that
        keyframe slot as keyframe_set_depth would. Returns dict(depth, var (f32), views, status (u8; REFINE_STATUS names the values),
        stats = the fields of ellc_refine_stats). The order of the views enters the result."""
        return self._refine("ellc_keyframe_refine_depth", (), kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, max_var, min_support,
                            support_k2, stride, params)

    # ---- hypotheses created in a keyframe's map by a depth sweep against other views
    def _sweep(self, name, tail, kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, params):
        B, vs, T, li, (rows, cols) = self._views_args(view_slots, Ts, lights, level)
        prm = params if isinstance(params, EllcSweepParams) else sweep_params(**(params or {}))
        depth, var = np.zeros((rows, cols), np.float32), np.zeros((rows, cols), np.float32)
        views, status = np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8)
        st = EllcSweepStats()
        self._ck(getattr(self._l, name)(self.h, int(kf_slot), int(level), B, int(views_are_keyframes), _p(vs), _p(T), _p(li), C.byref(prm), int(dst_slot),
                                        _p(depth), _p(var), _p(views), _p(status), C.byref(st), *tail), name)
        return depth, var, views, status, {k: getattr(st, k) for k in SWEEP_STATS_FIELDS}

    def sweep_depth(self, kf_slot, view_slots, Ts, lights=None, level=0, views_are_keyframes=True, dst_slot=-1, params=None):
        """Hypotheses for the pixels of keyframe slot kf_slot that hold none, from a sweep over inverse depths against the images of the
        views (ellc_keyframe_sweep_depth): view_slots, Ts, lights, level, views_are_keyframes and dst_slot as in refine_depth. params: an
        ellc_sweep_params (sweep_params()) or a dict of sigma_i2, huber_k, d_min, d_max, min_grad2, max_cost, distinct_ratio, var_scale,
        n_samples, min_views (defaults 16, 1.345, 0.125, 4, 100, 0, 0.7, 1, 64, 2). Returns (depth, var (f32), views, status (u8;
        SWEEP_STATUS names the values), stats = the fields of ellc_sweep_stats as a dict)."""
        return self._sweep("ellc_keyframe_sweep_depth", (), kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, params)

    # ---- the hypotheses of a keyframe's map that other views contradict, removed
    def _cull(self, name, tail, kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, max_var, min_support, support_k2, stride, params):
        B, vs, T, li, (rows, cols), flt = self._views_args(view_slots, Ts, lights, level, (max_var, min_support, support_k2, stride))
        prm = params if isinstance(params, EllcCullParams) else cull_default_params(**(params or {}))
        res = dict(depth=np.zeros((rows, cols), np.float32), var=np.zeros((rows, cols), np.float32), votes=np.zeros((rows, cols), np.uint32),
                   photo=np.zeros((rows, cols), np.uint8), status=np.zeros((rows, cols), np.uint8))
        st = EllcCullStats()
        self._ck(getattr(self._l, name)(self.h, int(kf_slot), int(level), B, int(views_are_keyframes), _p(vs), _p(T), _p(li), C.byref(flt), C.byref(prm),
                                        int(dst_slot), _p(res["depth"]), _p(res["var"]), _p(res["votes"]), _p(res["photo"]), _p(res["status"]),
                                        C.byref(st), *tail), name)
        res["stats"] = {k: getattr(st, k) for k in CULL_STATS_FIELDS}
        return res

    def cull_depth(self, kf_slot, view_slots, Ts, lights=None, level=0, views_are_keyframes=True, dst_slot=-1, max_var=0.0, min_support=0,
                   support_k2=1.0, stride=1, params=None):
        """The hypotheses of keyframe slot kf_slot that the views contradict, removed (ellc_keyframe_cull_depth): view_slots, Ts, lights,
        level, views_are_keyframes, dst_slot and the filter as in refine_depth. A keyframe view that holds a depth votes geometrically
        (agree / in front / behind, depth_consistency's rule) and photometrically, every other view photometrically only. params: an
        ellc_cull_params (cull_default_params()) or a dict of agree_k2, sigma_i2, photo_k, min_support, min_judged, min_in_front,
        min_photo (defaults 1, 16, 3, 1, 2, 1, 2; photo_k <= 0: no photometric vote). Returns dict(depth, var (f32; a culled pixel is
        0 / -1, every other keeps the slot's bits), votes (u32: agree | in_front << 8 | behind << 16 | photo_bad << 24), photo, status
        (u8; CULL_STATUS names the values), stats = the fields of ellc_cull_stats). The order of the views does not enter the result."""
        return self._cull("ellc_keyframe_cull_depth", (), kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, max_var, min_support,
                          support_k2, stride, params)

    # ---- poses and depths refined in one step
    def _joint_args(self, view_slots, Ts, lights, level, max_var, min_support, support_k2, stride, params, inv_depth):
        B, vs, T, li, shape, flt = self._views_args(view_slots, Ts, lights, level, (max_var, min_support, support_k2, stride))
        prm = params if isinstance(params, EllcJointParams) else joint_default_params(**(params or {}))
        d = None if inv_depth is None else np.ascontiguousarray(inv_depth, np.float32).reshape(shape)
        return B, vs, T, li, flt, prm, d, shape

    @staticmethod
    def _joint_planes(shape):
        return dict(inv_depth=np.zeros(shape, np.float32), depth=np.zeros(shape, np.float32), var=np.zeros(shape, np.float32),
                    views=np.zeros(shape, np.uint8), status=np.zeros(shape, np.uint8))

    def joint_step(self, kf_slot, view_slots, Ts, lights=None, level=0, views_are_keyframes=True, inv_depth=None, max_var=0.0, min_support=0,
                   support_k2=1.0, stride=1, params=None, _profile=None):
        """The normal equations of one joint Gauss-Newton step over the SE(3) of the views and the inverse depths of keyframe slot
        kf_slot (ellc_keyframe_joint_step), the depths eliminated: kf_slot, view_slots, Ts, lights, level, views_are_keyframes and the
        filter as in refine_depth; inv_depth: the plane of inverse depths to evaluate at (None, or a value that is not > 0: the slot's
        own). params: an ellc_joint_params (joint_default_params()) or a dict of sigma_i2, huber_k, prior_weight, max_step_rel, min_views
        (defaults 16, 1.345, 1, 0.5, 2). Returns a 0-d structured array, one ellc_joint_normal: A, a per view, S, s of the Schur
        complement, chi2_photo, chi2_prior, the counts and B. joint_solve turns it into the views' pose steps."""
        B, vs, T, li, flt, prm, d, _ = self._joint_args(view_slots, Ts, lights, level, max_var, min_support, support_k2, stride, params, inv_depth)
        out = np.zeros(1, JOINT_NORMAL_DTYPE)
        name = "ellc_profile_joint_step" if _profile is not None else "ellc_keyframe_joint_step"
        tail = (C.byref(_profile),) if _profile is not None else ()
        self._ck(getattr(self._l, name)(self.h, int(kf_slot), int(level), B, int(views_are_keyframes), _p(vs), _p(T), _p(li), C.byref(flt), C.byref(prm),
                                        _p(d), _p(out), *tail), name)
        return out[0]

    def joint_apply(self, kf_slot, view_slots, Ts, xi, lights=None, level=0, views_are_keyframes=True, inv_depth=None, dst_slot=-1, max_var=0.0,
                    min_support=0, support_k2=1.0, stride=1, params=None, _profile=None):
        """The joint step taken (ellc_keyframe_joint_apply): xi is [B][6] f64, rotation then translation per view, as joint_solve returns
        it. Returns dict(T = [B][12] f32 the moved transforms, inv_depth, depth, var (f32), views, status (u8; JOINT_STATUS names the
        values), stats = the fields of ellc_joint_apply_stats). var is the variance CONDITIONAL on the poses (optimistic). dst_slot >= 0
        (level 0 only) stores depth and var into that keyframe slot as keyframe_set_depth would."""
        B, vs, T, li, flt, prm, d, shape = self._joint_args(view_slots, Ts, lights, level, max_var, min_support, support_k2, stride, params, inv_depth)
        x = np.ascontiguousarray(xi, np.float64).reshape(6 * B)
        res = self._joint_planes(shape)
        res["T"] = np.zeros((B, 12), np.float32)
        st = EllcJointApplyStats()
        name = "ellc_profile_joint_apply" if _profile is not None else "ellc_keyframe_joint_apply"
        tail = (C.byref(_profile),) if _profile is not None else ()
        self._ck(getattr(self._l, name)(self.h, int(kf_slot), int(level), B, int(views_are_keyframes), _p(vs), _p(T), _p(li), C.byref(flt), C.byref(prm),
                                        _p(d), _p(x), int(dst_slot), _p(res["T"]), _p(res["inv_depth"]), _p(res["depth"]), _p(res["var"]),
                                        _p(res["views"]), _p(res["status"]), C.byref(st), *tail), name)
        res["stats"] = {f[0]: getattr(st, f[0]) for f in EllcJointApplyStats._fields_ if f[0] != "reserved"}
        return res

    def joint_refine(self, kf_slot, view_slots, Ts, lights=None, level=0, views_are_keyframes=True, inv_depth=None, max_iter=6, eps=1e-6, lam=0.0,
                     dst_slot=-1, max_var=0.0, min_support=0, support_k2=1.0, stride=1, params=None, trace=False):
        """The loop over joint_step, joint_solve and joint_apply (ellc_keyframe_joint_refine): a trial state is accepted iff the next
        step's (chi2_photo + chi2_prior) / (n_terms + n_used) did not rise; a refused trial, a refused solve or max |xi| < eps ends the
        loop at the last accepted state. lam: the factor (1 + lam) on the reduced matrix's diagonal. Returns dict(T, rec, iters and the
        five planes of joint_apply) and, with trace=True, trace_T, trace_rec, trace_xi, trace_accepted over the steps made."""
        B, vs, T, li, flt, prm, d, shape = self._joint_args(view_slots, Ts, lights, level, max_var, min_support, support_k2, stride, params, inv_depth)
        cap = max(int(max_iter), 1) + 1
        res = self._joint_planes(shape)
        res.update(T=np.zeros((B, 12), np.float32), rec=np.zeros(1, JOINT_NORMAL_DTYPE))
        iters = C.c_int(0)
        tr = dict(trace_T=np.zeros((cap, B, 12), np.float32), trace_rec=np.zeros(cap, JOINT_NORMAL_DTYPE), trace_xi=np.zeros((cap, B, 6), np.float64),
                  trace_accepted=np.zeros(cap, np.int32)) if trace else {}
        name = "ellc_keyframe_joint_refine"
        self._ck(getattr(self._l, name)(self.h, int(kf_slot), int(level), B, int(views_are_keyframes), _p(vs), _p(T), _p(li), C.byref(flt), C.byref(prm),
                                        _p(d), int(max_iter), C.c_float(eps), C.c_double(lam), int(dst_slot), _p(res["T"]), _p(res["rec"]),
                                        C.byref(iters), _p(res["inv_depth"]), _p(res["depth"]), _p(res["var"]), _p(res["views"]), _p(res["status"]),
                                        _p(tr.get("trace_T")), _p(tr.get("trace_rec")), _p(tr.get("trace_xi")), _p(tr.get("trace_accepted")),
                                        cap if trace else 0), name)
        res["rec"] = res["rec"][0]
        res["iters"] = iters.value
        if trace:
            n = int((tr["trace_rec"]["n_kept"] >= 0).sum())
            res.update({k: v[:n].copy() for k, v in tr.items()})
        return res

    def profile_joint_step(self, *args, **kw):
        """joint_step through ellc_profile_joint_step: (record, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_joint_step")
        ms = C.c_float(0.0)
        return self.joint_step(*args, _profile=ms, **kw), ms.value

    def profile_joint_apply(self, *args, **kw):
        """joint_apply through ellc_profile_joint_apply: (result, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_joint_apply")
        ms = C.c_float(0.0)
        return self.joint_apply(*args, _profile=ms, **kw), ms.value

    # ---- measurement hooks, self-tests, test hooks: contexts created with diag=True only (include/ellc_abi_diag.h)
    def _need_diag(self, what):
        if not self.diag and _lib.DIAG_SO_PATH != _lib.SO_PATH:
            raise EllcError("%s is a diagnostic entry point (include/ellc_abi_diag.h): create the context with diag=True" % what)

    def debug_persist_delay(self, first_block, polls):
        self._need_diag("ellc_debug_persist_delay")
        self._ck(self._l.ellc_debug_persist_delay(self.h, int(first_block), int(polls)), "ellc_debug_persist_delay")

    def debug_set_persist_epoch(self, epoch):
        self._need_diag("ellc_debug_set_persist_epoch")
        self._ck(self._l.ellc_debug_set_persist_epoch(self.h, C.c_uint(epoch)), "ellc_debug_set_persist_epoch")

    def debug_set_eager_lists(self, on):
        self._need_diag("ellc_debug_set_eager_lists")
        self._ck(self._l.ellc_debug_set_eager_lists(self.h, int(bool(on))), "ellc_debug_set_eager_lists")

    def debug_set_fold_staging(self, on):
        self._need_diag("ellc_debug_set_fold_staging")
        self._ck(self._l.ellc_debug_set_fold_staging(self.h, int(bool(on))), "ellc_debug_set_fold_staging")

    def debug_set_hinv_cache(self, on):
        self._need_diag("ellc_debug_set_hinv_cache")
        self._ck(self._l.ellc_debug_set_hinv_cache(self.h, int(bool(on))), "ellc_debug_set_hinv_cache")

    def debug_set_count_cache(self, on):
        self._need_diag("ellc_debug_set_count_cache")
        self._ck(self._l.ellc_debug_set_count_cache(self.h, int(bool(on))), "ellc_debug_set_count_cache")

    def debug_set_mask_scatter(self, on):
        """1 (default): a launch group's compaction ranks its pixels from the kept valid-bit masks; 0: from the depth planes."""
        self._need_diag("ellc_debug_set_mask_scatter")
        self._ck(self._l.ellc_debug_set_mask_scatter(self.h, int(bool(on))), "ellc_debug_set_mask_scatter")

    def debug_mask_scatter_counters(self):
        """(scatter launches in the masked form, in the depth-reading form behind a count) enqueued or captured so far."""
        self._need_diag("ellc_debug_mask_scatter_counters")
        a = C.c_longlong(0); b = C.c_longlong(0)
        self._ck(self._l.ellc_debug_mask_scatter_counters(self.h, C.byref(a), C.byref(b)), "ellc_debug_mask_scatter_counters")
        return a.value, b.value

    def debug_get_valid_mask(self, kf_slot, level):
        """The valid-bit mask the last count launch left for a keyframe slot at `level`: a (tiles, 64) uint32 array, bit i of a
        tile = (depth > 0) of pixel tile * 2048 + i."""
        self._need_diag("ellc_debug_get_valid_mask")
        tiles = ((self.cfg.height >> level) * (self.cfg.width >> level) + 2047) // 2048
        out = np.zeros((tiles, 64), np.uint32)
        self._ck(self._l.ellc_debug_get_valid_mask(self.h, int(kf_slot), int(level), out.ctypes.data_as(C.c_void_p)), "ellc_debug_get_valid_mask")
        return out

    def debug_set_packed_taps(self, on):
        """Tolerance mode: 1 (default) the interior taps as one load from the row-packed plane, 0 as four row loads."""
        self._need_diag("ellc_debug_set_packed_taps")
        self._ck(self._l.ellc_debug_set_packed_taps(self.h, int(bool(on))), "ellc_debug_set_packed_taps")

    def debug_row_tap_launches(self):
        """Kernel argument records this context has built with the row loads selected (debug_set_packed_taps(False))."""
        self._need_diag("ellc_debug_row_tap_launches")
        n = C.c_longlong(0)
        self._ck(self._l.ellc_debug_row_tap_launches(self.h, C.byref(n)), "ellc_debug_row_tap_launches")
        return n.value

    def debug_get_packed_level(self, frame_slot, level):
        """The row-packed plane of a frame slot at `level` as a (stored_h, stored_w) uint32 array."""
        self._need_diag("ellc_debug_get_packed_level")
        sw = C.c_int(0); sh = C.c_int(0)
        self._ck(self._l.ellc_get_image_level(self.h, 0, int(frame_slot), int(level), None, C.byref(sw), C.byref(sh), None, None), "ellc_get_image_level")
        out = np.empty((sh.value, sw.value), np.uint32)
        self._ck(self._l.ellc_debug_get_packed_level(self.h, int(frame_slot), int(level), out.ctypes.data_as(C.c_void_p)), "ellc_debug_get_packed_level")
        return out

    def debug_count_cache_counters(self):
        """(groups that compacted with a count launch, groups that compacted without one) so far."""
        self._need_diag("ellc_debug_count_cache_counters")
        a = C.c_longlong(0); b = C.c_longlong(0)
        self._ck(self._l.ellc_debug_count_cache_counters(self.h, C.byref(a), C.byref(b)), "ellc_debug_count_cache_counters")
        return a.value, b.value

    def debug_persist_counters(self):
        self._need_diag("ellc_debug_persist_counters")
        a = C.c_longlong(0); b = C.c_longlong(0); r = C.c_longlong(0)
        self._ck(self._l.ellc_debug_persist_counters(self.h, C.byref(a), C.byref(b), C.byref(r)), "ellc_debug_persist_counters")
        return a.value, b.value, r.value

    def debug_schedule_sums(self, kf_slots, frame_slots, level, pose, mode=MODE_FCA):
        """One launch of the level-bound schedule's kernel at `level` from the poses pose[b] (ellc_debug_schedule_sums). Returns
        dict(H=[B][6][6] symmetric, b=[B][6] (f64, the blocks' sums), pose=[B][6] after the step, hinv=[B][6][6] (constant-weight
        path), kernel=name, grid=(blocks per alignment, age rounds, xcd relabelling))."""
        self._need_diag("ellc_debug_schedule_sums")
        B = len(kf_slots)
        pose = np.ascontiguousarray(np.broadcast_to(np.asarray(pose, np.float32).reshape(-1, 6), (B, 6)), np.float32)
        _, kf, fr, _ = self._batch(kf_slots, frame_slots, None)
        sums = np.zeros((B, 27), np.float64); newp = np.zeros((B, 6), np.float32); hinv = np.zeros((B, 36), np.float32)
        name = C.create_string_buffer(64); grid = np.zeros(3, np.int32)
        self._ck(self._l.ellc_debug_schedule_sums(self.h, B, _p(kf), _p(fr), level, mode, _p(pose), _p(sums), _p(newp), _p(hinv), name, 64,
                                                  _p(grid)), "ellc_debug_schedule_sums")
        H = np.zeros((B, 6, 6), np.float64)
        iu = np.triu_indices(6)
        H[:, iu[0], iu[1]] = sums[:, :21]
        H[:, iu[1], iu[0]] = sums[:, :21]
        return dict(H=H, b=sums[:, 21:].copy(), pose=newp, hinv=hinv.reshape(B, 6, 6), kernel=name.value.decode(),
                    grid=tuple(int(v) for v in grid))

    def profile_gn_kernel(self, kf_slots, frame_slots, level, reps=20):
        self._need_diag("ellc_profile_gn_kernel")
        B, kf, fr, _ = self._batch(kf_slots, frame_slots, None)
        ms = C.c_float(0); by = C.c_double(0); v = C.c_longlong(0)
        self._ck(self._l.ellc_profile_gn_kernel(self.h, B, _p(kf), _p(fr), level, reps, C.byref(ms), C.byref(by), C.byref(v)),
                 "ellc_profile_gn_kernel")
        return ms.value, by.value, v.value

    def selftest_div_pair(self, a, b):
        self._need_diag("ellc_selftest_div_pair")
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        qp = np.zeros_like(a); qr = np.zeros_like(a)
        self._ck(self._l.ellc_selftest_div_pair(self.h, int(a.size), _p(a), _p(b), _p(qp), _p(qr)), "ellc_selftest_div_pair")
        return qp, qr

    def selftest_lu(self, tri21):
        self._need_diag("ellc_selftest_lu")
        tri21 = np.ascontiguousarray(tri21, np.float64).reshape(-1, 21)
        out = np.zeros((tri21.shape[0], 6, 6), np.float32)
        self._ck(self._l.ellc_selftest_lu(self.h, int(tri21.shape[0]), _p(tri21), _p(out)), "ellc_selftest_lu")
        return out

    def profile_map_points(self, kf_slots, T12, level=0, max_var=0.0, min_support=0, support_k2=1.0, stride=1):
        """map_points through ellc_profile_map_points: (points, counts, device ms of the three launches)."""
        self._need_diag("ellc_profile_map_points")
        kf = np.ascontiguousarray(kf_slots, np.int32).reshape(-1)
        B = kf.size
        T = np.ascontiguousarray(T12, np.float32).reshape(B, 12)
        flt = EllcMapFilter(max_var, int(min_support), support_k2, int(stride))
        counts = np.zeros(B, np.int32); total = C.c_int(0); ms = C.c_float(0)
        self._ck(self._l.ellc_profile_map_points(self.h, B, _p(kf), _p(T), int(level), C.byref(flt), None, 0, _p(counts), C.byref(total), C.byref(ms)),
                 "ellc_profile_map_points")
        pts = np.zeros(total.value, MAP_POINT_DTYPE)
        self._ck(self._l.ellc_profile_map_points(self.h, B, _p(kf), _p(T), int(level), C.byref(flt), _p(pts), total.value, _p(counts), C.byref(total),
                                                 C.byref(ms)), "ellc_profile_map_points")
        return pts, counts, ms.value

    def profile_render_depth(self, kf_slots, T12, level=0, agree_k2=1.0, dst_slot=-1, max_var=0.0, min_support=0, support_k2=1.0, stride=1, out=None):
        """render_depth through ellc_profile_render_depth: its dict plus launches_ms, the device time of the launches."""
        self._need_diag("ellc_profile_render_depth")
        ms = C.c_float(0)
        out = self._render(self._l.ellc_profile_render_depth, "ellc_profile_render_depth", (C.byref(ms),), kf_slots, T12, level, agree_k2,
                           dst_slot, max_var, min_support, support_k2, stride, out)
        out["launches_ms"] = ms.value
        return out

    def profile_fuse_depth(self, kf_slots, T12, level=0, agree_k2=1.0, max_merge=64, dst_slot=-1, max_var=0.0, min_support=0, support_k2=1.0,
                           stride=1, out=None):
        """fuse_depth through ellc_profile_fuse_depth: its dict plus launches_ms, the device time of the launches (the host's read of the
        list's size lies inside it)."""
        self._need_diag("ellc_profile_fuse_depth")
        ms = C.c_float(0)
        out = self._fuse(self._l.ellc_profile_fuse_depth, "ellc_profile_fuse_depth", (C.byref(ms),), kf_slots, T12, level, agree_k2, max_merge,
                         dst_slot, max_var, min_support, support_k2, stride, out)
        out["launches_ms"] = ms.value
        return out

    def profile_depth_absorb(self, kf_slots, T12, params=None, max_var=0.0, min_support=0, support_k2=1.0, stride=1, stats=None):
        """depth_absorb through ellc_profile_depth_absorb: its dict plus launches_ms, the device time of the fold's launches (the host's
        read of the list's size lies inside it; finalise's launches do not)."""
        self._need_diag("ellc_profile_depth_absorb")
        ms = C.c_float(0)
        out = self._absorb(self._l.ellc_profile_depth_absorb, "ellc_profile_depth_absorb", (C.byref(ms),), kf_slots, T12, params, max_var,
                           min_support, support_k2, stride, stats)
        out["launches_ms"] = ms.value
        return out

    def profile_trial_propagate(self, src_slots, dst_slots, Ts, dst_is_keyframe=False, photo_gate=1, max_group_requests=0, max_var=0.0,
                                min_support=0, support_k2=1.0, stride=1):
        """trial_propagate through ellc_profile_trial_propagate: (records, launches_ms), with the number of requests per launch forced
        to max_group_requests (0: the product call's choice). The records do not depend on it."""
        self._need_diag("ellc_profile_trial_propagate")
        ms = C.c_float(0.0)
        out = self._trial(self._l.ellc_profile_trial_propagate, "ellc_profile_trial_propagate", (int(max_group_requests), C.byref(ms)), src_slots,
                          dst_slots, Ts, dst_is_keyframe, photo_gate, max_var, min_support, support_k2, stride)
        return out, float(ms.value)

    def profile_depth_consistency(self, src_slots, dst_slots, Ts, level=0, agree_k2=1.0, max_var=0.0, min_support=0, support_k2=1.0, stride=1):
        """depth_consistency through ellc_profile_depth_consistency: (records, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_depth_consistency")
        ms = C.c_float(0)
        out = self._consistency(self._l.ellc_profile_depth_consistency, "ellc_profile_depth_consistency", (C.byref(ms),), src_slots, dst_slots, Ts,
                                level, agree_k2, max_var, min_support, support_k2, stride)
        return out, ms.value

    def profile_sim3_step(self, src_slots, dst_slots, Ts, level=0, max_var=0.0, min_support=0, support_k2=1.0, stride=1, params=None):
        """sim3_step through ellc_profile_sim3_step: (records, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_sim3_step")
        ms = C.c_float(0)
        out = self._pair_step("ellc_profile_sim3_step", SIM3_NORMAL_DTYPE, (), src_slots, dst_slots, Ts, level, max_var, min_support, support_k2, stride,
                              params, tail=(C.byref(ms),))
        return out, ms.value

    def profile_light_step(self, src_slots, dst_slots, Ts, lights=None, **kw):
        """light_step through ellc_profile_light_step: (records, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_light_step")
        ms = C.c_float(0)
        out = self._pair_step("ellc_profile_light_step", LIGHT_NORMAL_DTYPE, (lights,), src_slots, dst_slots, Ts, tail=(C.byref(ms),), **kw)
        return out, ms.value

    def profile_sim3_step_lit(self, src_slots, dst_slots, Ts, lights=None, **kw):
        """sim3_step_lit through ellc_profile_sim3_step_lit: (records, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_sim3_step_lit")
        ms = C.c_float(0)
        out = self._pair_step("ellc_profile_sim3_step_lit", SIM3_NORMAL_DTYPE, (lights,), src_slots, dst_slots, Ts, tail=(C.byref(ms),), **kw)
        return out, ms.value

    def profile_refine_depth(self, kf_slot, view_slots, Ts, lights=None, level=0, views_are_keyframes=True, dst_slot=-1, max_var=0.0, min_support=0,
                             support_k2=1.0, stride=1, params=None):
        """refine_depth through ellc_profile_refine_depth: (result, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_refine_depth")
        ms = C.c_float(0)
        out = self._refine("ellc_profile_refine_depth", (C.byref(ms),), kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, max_var,
                           min_support, support_k2, stride, params)
        return out, ms.value

    def profile_sweep_depth(self, kf_slot, view_slots, Ts, lights=None, level=0, views_are_keyframes=True, dst_slot=-1, params=None):
        """sweep_depth through ellc_profile_sweep_depth: (result, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_sweep_depth")
        ms = C.c_float(0)
        out = self._sweep("ellc_profile_sweep_depth", (C.byref(ms),), kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, params)
        return out, ms.value

    def profile_cull_depth(self, kf_slot, view_slots, Ts, lights=None, level=0, views_are_keyframes=True, dst_slot=-1, max_var=0.0, min_support=0,
                           support_k2=1.0, stride=1, params=None):
        """cull_depth through ellc_profile_cull_depth: (result, launches_ms), the device time of the launches."""
        self._need_diag("ellc_profile_cull_depth")
        ms = C.c_float(0)
        out = self._cull("ellc_profile_cull_depth", (C.byref(ms),), kf_slot, view_slots, Ts, lights, level, views_are_keyframes, dst_slot, max_var,
                         min_support, support_k2, stride, params)
        return out, ms.value

    def profile_calibrate_read(self, nbytes, reps=10):
        self._need_diag("ellc_profile_calibrate_read")
        ms = C.c_float(0)
        self._ck(self._l.ellc_profile_calibrate_read(self.h, C.c_size_t(nbytes), reps, C.byref(ms)), "ellc_profile_calibrate_read")
        return ms.value

    def profile_depth_stage(self, stage, frame_slot, pose, reps=20):
        """ms per call of one depth-map stage (0 regularize, 1 fill holes, 2 observe, 3 update depth image, 4 createKeyFrame's
        regularise + fill + regularise in one launch, 5 the tracked frame's fill + regularise + update depth image in one launch),
        HIP events."""
        self._need_diag("ellc_profile_depth_stage")
        pose = np.ascontiguousarray(pose, np.float32)
        ms = C.c_float(0)
        self._ck(self._l.ellc_profile_depth_stage(self.h, stage, frame_slot, _p(pose), reps, C.byref(ms)), "ellc_profile_depth_stage")
        return ms.value

    def profile_stream_read(self, nbytes, reps=10):
        self._need_diag("ellc_profile_stream_read")
        ms = C.c_float(0)
        self._ck(self._l.ellc_profile_stream_read(self.h, C.c_size_t(nbytes), reps, C.byref(ms)), "ellc_profile_stream_read")
        return ms.value

    def profile_align(self, kf_slots, frame_slots, init_pose=None, mode=MODE_FCA, reps=5):
        self._need_diag("ellc_profile_align")
        B, kf, fr, ip = self._batch(kf_slots, frame_slots, init_pose)
        ms = C.c_float(0)
        self._ck(self._l.ellc_profile_align(self.h, B, _p(kf), _p(fr), _p(ip), mode, reps, C.byref(ms)), "ellc_profile_align")
        return ms.value


def copy_slot_across(dst_ctx, dst_is_kf, dst, src_ctx, src_is_kf, src):
    """ellc_copy_slot_across: a slot's planes from one context into another on the same device (the loop-closure ring's deep copy)."""
    if dst_ctx._l is not src_ctx._l:
        raise EllcError("ellc_copy_slot_across: the two contexts live in different libraries")
    st = dst_ctx._l.ellc_copy_slot_across(dst_ctx.h, int(dst_is_kf), dst, src_ctx.h, int(src_is_kf), src)
    if st != 0:
        raise EllcError("ellc_copy_slot_across -> %d: %s" % (st, dst_ctx._l.ellc_last_error(dst_ctx.h).decode()))


def concatenate_relative_pose(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    o = np.zeros(6, np.float32)
    _lib.lib().ellc_concatenate_relative_pose(_p(a), _p(b), _p(o))
    return o


def concatenate_origin_pose(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    o = np.zeros(6, np.float32)
    _lib.lib().ellc_concatenate_origin_pose(_p(a), _p(b), _p(o))
    return o


def se3_exp(pose):
    p = np.ascontiguousarray(pose, np.float32)
    T = np.zeros(16, np.float32)
    _lib.lib().ellc_se3_exp(_p(p), _p(T))
    return T.reshape(4, 4)


def se3_log(T):
    T = np.ascontiguousarray(T, np.float32).reshape(16)
    p = np.zeros(6, np.float32)
    _lib.lib().ellc_se3_log(_p(T), _p(p))
    return p


def sim3_params(sigma_i2=None, huber_k=None, gate_k2=None, depth_weight=None):
    """ellc_sim3_params: the library's defaults (ellc_sim3_default_params) with the given fields replaced."""
    p = EllcSim3Params()
    _lib.lib().ellc_sim3_default_params(C.byref(p))
    for k, v in (("sigma_i2", sigma_i2), ("huber_k", huber_k), ("gate_k2", gate_k2), ("depth_weight", depth_weight)):
        if v is not None:
            setattr(p, k, v)
    return p


def light_params(gain_min=None, gain_max=None, min_pixels=None):
    """ellc_light_params: the library's defaults (ellc_light_default_params) with the given fields replaced."""
    p = EllcLightParams()
    _lib.lib().ellc_light_default_params(C.byref(p))
    for k, v in (("gain_min", gain_min), ("gain_max", gain_max), ("min_pixels", min_pixels)):
        if v is not None:
            setattr(p, k, v)
    return p


def refine_default_params(sigma_i2=None, huber_k=None, prior_weight=None, max_step_rel=None, n_iter=None, min_views=None):
    """ellc_refine_params: the library's defaults (ellc_refine_default_params) with the given fields replaced."""
    p = EllcRefineParams()
    _lib.lib().ellc_refine_default_params(C.byref(p))
    for k, v in (("sigma_i2", sigma_i2), ("huber_k", huber_k), ("prior_weight", prior_weight), ("max_step_rel", max_step_rel), ("n_iter", n_iter),
                 ("min_views", min_views)):
        if v is not None:
            setattr(p, k, v)
    return p


def sweep_params(sigma_i2=None, huber_k=None, d_min=None, d_max=None, min_grad2=None, max_cost=None, distinct_ratio=None, var_scale=None,
                 n_samples=None, min_views=None):
    """ellc_sweep_params: the library's defaults (ellc_sweep_default_params) with the given fields replaced."""
    p = EllcSweepParams()
    _lib.lib().ellc_sweep_default_params(C.byref(p))
    for k, v in (("sigma_i2", sigma_i2), ("huber_k", huber_k), ("d_min", d_min), ("d_max", d_max), ("min_grad2", min_grad2), ("max_cost", max_cost),
                 ("distinct_ratio", distinct_ratio), ("var_scale", var_scale), ("n_samples", n_samples), ("min_views", min_views)):
        if v is not None:
            setattr(p, k, v)
    return p


def cull_default_params(agree_k2=None, sigma_i2=None, photo_k=None, min_support=None, min_judged=None, min_in_front=None, min_photo=None):
    """ellc_cull_params: the library's defaults (ellc_cull_default_params) with the given fields replaced."""
    p = EllcCullParams()
    _lib.lib().ellc_cull_default_params(C.byref(p))
    for k, v in (("agree_k2", agree_k2), ("sigma_i2", sigma_i2), ("photo_k", photo_k), ("min_support", min_support), ("min_judged", min_judged),
                 ("min_in_front", min_in_front), ("min_photo", min_photo)):
        if v is not None:
            setattr(p, k, v)
    return p


def sim3_invert(T12, light=None):
    """ellc_sim3_invert: (the inverse of a row-major 3x4 similarity as 12 f32, the inverse light (1 / gain, -offset / gain) as 2 f32);
    light None means (1, 0)."""
    T = np.ascontiguousarray(T12, np.float32).reshape(12)
    li = None if light is None else np.ascontiguousarray(light, np.float32).reshape(2)
    To, lo = np.zeros(12, np.float32), np.zeros(2, np.float32)
    _lib.lib().ellc_sim3_invert(_p(T), _p(li), _p(To), _p(lo))
    return To, lo


def _as_light_params(p):
    return p if isinstance(p, EllcLightParams) else light_params(**(p or {}))


def light_solve(rec, light_in=None, params=None):
    """ellc_light_solve of one ellc_light_normal record (a row of light_step's array): (light f32 [2], refused). params: an
    ellc_light_params (light_params()) or a dict of its fields; light_in None means (1, 0)."""
    r = np.ascontiguousarray(np.asarray(rec, LIGHT_NORMAL_DTYPE).reshape(1))
    p = _as_light_params(params)
    li = None if light_in is None else np.ascontiguousarray(light_in, np.float32).reshape(2)
    out = np.zeros(2, np.float32)
    refused = _lib.lib().ellc_light_solve(_p(r), C.byref(p), _p(li), _p(out))
    return out, bool(refused)


def trial_light_solve(rec, light_in=None, params=None):
    """ellc_trial_light_solve of one ellc_trial_propagation_lit record (a row of trial_propagate_lit's array): the unweighted fit of Iw on
    Is over its interior pixels, by light_solve's rule: (light f32 [2], refused)."""
    r = np.ascontiguousarray(np.asarray(rec, TRIAL_LIT_DTYPE).reshape(1))
    p = _as_light_params(params)
    li = None if light_in is None else np.ascontiguousarray(light_in, np.float32).reshape(2)
    out = np.zeros(2, np.float32)
    refused = _lib.lib().ellc_trial_light_solve(_p(r), C.byref(p), _p(li), _p(out))
    return out, bool(refused)


def absorb_params(agree_k2=None, max_fold=None, photo_gate=None, src_validity=None, finalise=None):
    """ellc_absorb_params: the library's defaults (ellc_absorb_default_params) with the given fields replaced."""
    p = EllcAbsorbParams()
    _lib.lib().ellc_absorb_default_params(C.byref(p))
    for k, v in (("agree_k2", agree_k2), ("max_fold", max_fold), ("photo_gate", photo_gate), ("src_validity", src_validity), ("finalise", finalise)):
        if v is not None:
            setattr(p, k, v)
    return p


def joint_default_params(sigma_i2=None, huber_k=None, prior_weight=None, max_step_rel=None, min_views=None):
    """ellc_joint_params: the library's defaults (ellc_joint_default_params) with the given fields replaced."""
    p = EllcJointParams()
    _lib.lib().ellc_joint_default_params(C.byref(p))
    for k, v in (("sigma_i2", sigma_i2), ("huber_k", huber_k), ("prior_weight", prior_weight), ("max_step_rel", max_step_rel), ("min_views", min_views)):
        if v is not None:
            setattr(p, k, v)
    return p


def joint_solve(rec, lam=0.0):
    """ellc_joint_solve of one ellc_joint_normal record: (xi [B][6] f64, refused). A refused solve leaves xi as zeros."""
    r = np.ascontiguousarray(np.asarray(rec, JOINT_NORMAL_DTYPE).reshape(1))
    B = int(r["B"][0])
    xi = np.zeros(6 * min(max(B, 1), JOINT_MAX_VIEWS), np.float64)
    refused = _lib.lib().ellc_joint_solve(_p(r), C.c_double(lam), _p(xi))
    return xi.reshape(-1, 6), bool(refused)


def sim3_solve(rec):
    """ellc_sim3_solve of one ellc_sim3_normal record (a row of sim3_step's array): (xi7 f64, singular)."""
    r = np.ascontiguousarray(np.asarray(rec, SIM3_NORMAL_DTYPE).reshape(1))
    xi = np.zeros(7, np.float64)
    singular = _lib.lib().ellc_sim3_solve(_p(r), _p(xi))
    return xi, bool(singular)


def sim3_apply(xi7, T12):
    """ellc_sim3_apply: float(exp(xi^) * T) with the generator [[w]x + sigma I, v; 0 0], as 12 f32."""
    xi = np.ascontiguousarray(xi7, np.float64).reshape(7)
    T = np.ascontiguousarray(T12, np.float32).reshape(12)
    out = np.zeros(12, np.float32)
    _lib.lib().ellc_sim3_apply(_p(xi), _p(T), _p(out))
    return out


def kl_divergence(p, q):
    p = np.ascontiguousarray(p, np.float32); q = np.ascontiguousarray(q, np.float32)
    return float(_lib.lib().ellc_kl_divergence(_p(p), _p(q), p.size))
