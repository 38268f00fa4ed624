"""Host-side mirror of the reference's MaskFusion / Model interface for the hot path.

Names and argument meaning follow Core/MaskFusion.h:45-307 and Core/Model/Model.h:108-268 of
martinruenz/maskfusion, over the C ABI in include/maskfusion_amd.h.  numpy arrays stand in for cv::Mat /
Eigen::Matrix4f.  Errors raise MFError (the reference throws std::runtime_error / exits on CUDA errors).
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from .lib import (load, MFError, Config, ModelInfo, InactiveInfo, RenderView, SessionInfo, MF_N_TIMINGS, TIMING_LABELS, MF_N_PASSES, PASS_LABELS,
                  MF_STATE_CONTEXT_SECTIONS, MF_STATE_MODEL_SECTIONS)


class Model:
    """View of one surfel model (Core/Model/Model.h)."""

    def __init__(self, owner: "MaskFusion", index: int):
        self._o = owner
        self._i = index

    def info(self) -> ModelInfo:
        out = ModelInfo()
        self._o._chk(self._o._L.mf_model_info(self._o._h, self._i, C.byref(out)))
        return out

    def getID(self) -> int:
        return int(self.info().id)

    def getClassID(self) -> int:
        return int(self.info().class_id)

    def getConfidenceThreshold(self) -> float:
        return float(self.info().confidence_threshold)

    def getPose(self) -> np.ndarray:
        out = np.zeros(16, np.float32)
        self._o._chk(self._o._L.mf_get_pose(self._o._h, self._i, out.ctypes.data))
        return out.reshape(4, 4).T.astype(np.float64)

    def lastCount(self) -> int:
        n = C.c_uint32(0)
        self._o._chk(self._o._L.mf_get_surfel_count(self._o._h, self._i, C.byref(n)))
        return int(n.value)

    def downloadMap(self) -> np.ndarray:
        """Model::downloadMap -> (count, 12) float32: pos+conf | colour,unused,initTime,lastTime | normal+radius."""
        n = self.lastCount()
        out = np.zeros((max(n, 1), 12), np.float32)
        cnt = C.c_uint32(0)
        self._o._chk(self._o._L.mf_download_map(self._o._h, self._i, out.ctypes.data, n, C.byref(cnt)))
        return out[:n]

    def getICPStats(self):
        e, c = C.c_float(0), C.c_float(0)
        self._o._chk(self._o._L.mf_get_icp_stats(self._o._h, self._i, C.byref(e), C.byref(c)))
        return e.value, c.value

    # -- the per-model operations of Core/Model/Model.h:126-162,233-268, on the frame staged with MaskFusion.stageFrame ----
    def initialise(self):
        self._o._chk(self._o._L.mf_model_initialise(self._o._h, self._i))

    def overridePose(self, pose):
        p = np.ascontiguousarray(np.asarray(pose, np.float32).T.reshape(16))
        self._o._chk(self._o._L.mf_model_override_pose(self._o._h, self._i, p.ctypes.data))

    def computeFusionWeight(self, weightMultiplier: float = 1.0) -> float:
        out = C.c_float(0)
        self._o._chk(self._o._L.mf_model_fusion_weight(self._o._h, self._i, weightMultiplier, C.byref(out)))
        return out.value

    def performTracking(self, frameToFrameRGB=False, rgbOnly=False, icpWeight=None, pyramid=True, fastOdom=False, so3=True,
                        maxDepthProcessed=20.0, logTimestamp=0, tryFillIn=False):
        # icpWeight=None: the weight the context was created with (the images a photometric term needs only exist if the context has one:
        # mf_model_perform_tracking returns MF_ESTATE otherwise instead of tracking against images that were never computed)
        if icpWeight is None:
            icpWeight = self._o.getParam("icpWeight")
        self._o._chk(self._o._L.mf_model_perform_tracking(self._o._h, self._i, int(frameToFrameRGB), int(rgbOnly), icpWeight,
                                                          int(pyramid), int(fastOdom), int(so3), maxDepthProcessed, logTimestamp,
                                                          int(tryFillIn)))

    def predictIndices(self, time: int, maxDepth: float, timeDelta: int):
        self._o._chk(self._o._L.mf_model_predict_indices(self._o._h, self._i, time, maxDepth, timeDelta))

    def fuse(self, time: int, depthCutoff: float, weightMultiplier: float = 1.0):
        self._o._chk(self._o._L.mf_model_fuse(self._o._h, self._i, time, depthCutoff, weightMultiplier))

    def clean(self, time: int, timeDelta: int, depthCutoff: float):
        self._o._chk(self._o._L.mf_model_clean(self._o._h, self._i, time, timeDelta, depthCutoff))

    def combinedPredict(self, maxDepth: float, time: int, maxTime: int, timeDelta: int):
        self._o._chk(self._o._L.mf_model_combined_predict(self._o._h, self._i, maxDepth, time, maxTime, timeDelta))

    def uploadMap(self, surfels: np.ndarray):
        s = np.ascontiguousarray(surfels, np.float32).reshape(-1, 12)
        self._o._chk(self._o._L.mf_model_upload_map(self._o._h, self._i, s.ctypes.data, len(s)))

    def mergeMap(self, source, T=None, radius=None, min_cos=None) -> list:
        """mf_model_merge_map: merges `source` ((n, 12) float32, downloadMap's layout) into this model's map on the GPU (DESIGN.md "Map
        merging").  T: 4 x 4, source frame -> the model's; radius: the partner search's (None: maskfusion_amd.merge.default_radius of the
        model's map); min_cos: the normal gate (None: merge.COS_HALF_RAD).  The model keeps its pose, age, id, class and static flag.
        Returns [averaged, confidence only, appended, dropped]; a merged map beyond the model's buffer raises and leaves the model as it was."""
        from . import merge as _merge
        s = np.ascontiguousarray(source, np.float32).reshape(-1, 12)
        radius = _merge.default_radius(self.downloadMap()) if radius is None else radius
        T16 = None if T is None else np.ascontiguousarray(np.asarray(T, np.float32).T.reshape(16))
        stats = (C.c_uint64 * 4)()
        self._o._chk(self._o._L.mf_model_merge_map(self._o._h, self._i, s.ctypes.data if len(s) else None, len(s),
                                                   T16.ctypes.data if T16 is not None else None, float(radius),
                                                   float(_merge.COS_HALF_RAD if min_cos is None else min_cos), stats))
        return [int(v) for v in stats]

    def makeNonStatic(self):
        self._o._chk(self._o._L.mf_make_nonstatic(self._o._h, self._i))

    def makeStatic(self):
        self._o._chk(self._o._L.mf_make_static(self._o._h, self._i))

    def isNonstatic(self) -> bool:
        return not bool(self.info().is_static)

    def debugRead(self, what: str) -> np.ndarray:
        return self._o.debugRead(what, model=self._i)


class MaskFusion:
    """MaskFusion facade (constructor arguments: Core/MaskFusion.h:47-53; Resolution/Intrinsics are explicit)."""

    def __init__(self, width=640, height=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, *, timeDelta=200,
                 initConfidenceGlobal=4.0, initConfidenceObject=2.0, depthCut=3.0, icpThresh=10.0, fastOdom=False,
                 so3=True, device=0, numGSurfels=9437184, numOSurfels=1048576, enableMultipleModels=True,
                 outlierCoefficient=0.9, modelSpawnOffset=20, trackAllModels=True, rgbOnly=False):
        self._L = load()
        cfg = Config()
        self._L.mf_default_config(C.byref(cfg), width, height, fx, fy, cx, cy)
        cfg.device = device
        cfg.time_delta = timeDelta
        cfg.conf_global = initConfidenceGlobal
        cfg.conf_object = initConfidenceObject
        cfg.depth_cutoff = depthCut
        cfg.icp_weight = icpThresh
        cfg.fast_odom = int(fastOdom)
        cfg.so3 = int(so3)
        cfg.rgb_only = int(rgbOnly)
        cfg.num_gsurfels = numGSurfels
        cfg.num_osurfels = numOSurfels
        cfg.enable_multiple_models = int(enableMultipleModels)
        cfg.outlier_coefficient = outlierCoefficient
        cfg.model_spawn_offset = modelSpawnOffset
        cfg.track_all_models = int(trackAllModels)
        self.cfg = cfg
        self.width, self.height = width, height
        h = C.c_void_p()
        rc = self._L.mf_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            why = {-1: "invalid configuration: width and height must be positive multiples of 8 (three pyramid levels), surfel capacities > 0",
                   -2: "needs a gfx950 GPU; there is no CPU path", -4: "out of device memory"}.get(rc, "see the HIP runtime's message on stderr")
            raise MFError(f"mf_create failed with code {rc} ({why})")
        self._h = h

    # -- lifetime -----------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.mf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            msg = self._L.mf_last_error(self._h)
            raise MFError(f"code {rc}: {msg.decode() if msg else ''}")

    # -- sessions (include/maskfusion_amd.h "Sessions"): a running context as a file, resumed bit for bit -------------------------
    def saveSession(self, path: str, user: bytes = b""):
        """Writes the context's state to `path` (read-only: nothing of the context changes); `user` is an opaque blob stored verbatim"""
        user = bytes(user)
        self._chk(self._L.mf_session_save(self._h, str(path).encode(), user if user else None, len(user)))

    @classmethod
    def loadSession(cls, path: str, device: int | None = None) -> "MaskFusion":
        """A new context that continues the saved one (on `device`; None: the device it was saved on)"""
        L = load()
        h = C.c_void_p()
        rc = L.mf_session_load(str(path).encode(), -1 if device is None else int(device), C.byref(h))
        if rc != 0:
            msg = L.mf_last_error(None)
            raise MFError(f"code {rc}: {msg.decode() if msg else ''}")
        self = cls.__new__(cls)
        self._L, self._h = L, h
        self.cfg = cls._sessionConfig(path)
        if device is not None:
            self.cfg.device = int(device)
        self.width, self.height = int(self.cfg.width), int(self.cfg.height)
        return self

    @staticmethod
    def _sessionConfig(path: str) -> Config:
        """the mf_config a session was saved with: its section "config", found through the section table (maskfusion_amd.h "Sessions")"""
        import struct
        with open(path, "rb") as f:
            head = f.read(64)
            table = f.read(64 * struct.unpack_from("<I", head, 48)[0])
            for i in range(len(table) // 64):
                name, owner, _, off, size, _ = struct.unpack_from("<32siIQQQ", table, 64 * i)
                if name.rstrip(b"\0") == b"config" and owner == -1 and size == C.sizeof(Config):
                    f.seek(off)
                    return Config.from_buffer_copy(f.read(size))
        raise MFError(f"{path}: no section config")

    @staticmethod
    def sessionInfo(path: str) -> dict:
        """Header and user blob of a session file; needs no GPU and creates no context"""
        L = load()
        out, n = SessionInfo(), C.c_uint64(0)
        rc = L.mf_session_info(str(path).encode(), C.byref(out), None, 0, C.byref(n))
        blob = C.create_string_buffer(max(int(n.value), 1))
        if rc == 0 and n.value:
            rc = L.mf_session_info(str(path).encode(), C.byref(out), blob, n.value, C.byref(n))
        if rc != 0:
            msg = L.mf_last_error(None)
            raise MFError(f"code {rc}: {msg.decode() if msg else ''}")
        d = {k: int(getattr(out, k)) for k in ("version", "width", "height", "n_models", "tick", "n_sections", "frames", "user_bytes", "file_bytes")}
        d["user"] = blob.raw[:int(n.value)]
        return d

    def stateDigest(self) -> dict:
        """One 64-bit word per device-resident section, computed on the device (mf_state_digest): context sections by name, a model's as
        "<name>[<index in the model list>]".  Equal states give equal words."""
        n = C.c_int32(0)
        cap = MF_STATE_CONTEXT_SECTIONS + 256 * MF_STATE_MODEL_SECTIONS
        out = np.zeros(cap, np.uint64)
        self._chk(self._L.mf_state_digest(self._h, out.ctypes.data, cap, C.byref(n)))
        names = [self._L.mf_state_section_name(i).decode() for i in range(MF_STATE_CONTEXT_SECTIONS + MF_STATE_MODEL_SECTIONS)]
        d = {}
        for j in range(n.value):
            if j < MF_STATE_CONTEXT_SECTIONS:
                d[names[j]] = int(out[j])
            else:
                m, k = divmod(j - MF_STATE_CONTEXT_SECTIONS, MF_STATE_MODEL_SECTIONS)
                d[f"{names[MF_STATE_CONTEXT_SECTIONS + k]}[{m}]"] = int(out[j])
        return d

    # -- MaskFusion::processFrame ---------------------------------------------------------------
    def processFrame(self, rgb: np.ndarray, depth: np.ndarray, mask: np.ndarray | None = None, timestamp: int = 0,
                     inPose=None, weightMultiplier: float = 1.0, bootstrap: bool = False, classIDs=()) -> bool:
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        assert rgb.shape == (self.height, self.width, 3) and depth.shape == (self.height, self.width)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
        pose = None
        if inPose is not None:
            pose = np.ascontiguousarray(np.asarray(inPose, np.float32).T.reshape(16))
        cid = np.ascontiguousarray(classIDs, np.int32) if len(classIDs) else None
        self._chk(self._L.mf_process_frame(self._h, rgb.ctypes.data, depth.ctypes.data,
                                           m.ctypes.data if m is not None else None,
                                           cid.ctypes.data if cid is not None else None, len(classIDs), timestamp,
                                           pose.ctypes.data if pose is not None else None, weightMultiplier,
                                           int(bootstrap)))
        if getattr(self, "_redetect", False):
            self.redetectModels(merge=getattr(self, "_redetect_merge", False))
        return False  # the reference always returns false (MaskFusion.cpp:606)

    def processFrameDevice(self, d_rgb: int, d_depth: int, d_mask: int = 0, timestamp: int = 0,
                           weightMultiplier: float = 1.0):
        """Inputs already resident in HBM (raw device pointers, e.g. torch tensor.data_ptr()); asynchronous."""
        self._chk(self._L.mf_process_frame_dev(self._h, d_rgb, d_depth, d_mask or None, timestamp, weightMultiplier))

    def setMaskClassIDs(self, classIDs):
        """FrameData::classIDs for the frames handed to processFrameDevice (class of mask value v = classIDs[v])"""
        a = np.ascontiguousarray(list(classIDs), np.int32)
        self._chk(self._L.mf_set_mask_class_ids(self._h, a.ctypes.data if len(a) else None, len(a)))

    def modelStateDevice(self, model: int, d_out16: int):
        """Enqueue a copy of {R, t, ICP error, inliers, surfels, alive} of `model` into a 16-float device buffer."""
        self._chk(self._L.mf_model_state_dev(self._h, model, d_out16))

    def sync(self):
        self._chk(self._L.mf_sync(self._h))

    def stageFrame(self, rgb: np.ndarray, depth: np.ndarray, mask: np.ndarray | None = None):
        """upload + filterDepth + Model::generateCUDATextures + intensity pyramid: what processFrame does before it touches a model"""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        m = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        self._chk(self._L.mf_stage_frame(self._h, rgb.ctypes.data, depth.ctypes.data, m.ctypes.data if m is not None else None))

    def stageFrameDevice(self, d_rgb: int, d_depth: int, d_mask: int = 0):
        """stageFrame for buffers already in device memory (pointers as integers), asynchronous: see mf_stage_frame_dev"""
        self._chk(self._L.mf_stage_frame_dev(self._h, d_rgb, d_depth, d_mask or None))

    def endFrame(self, timestamp: int = 0):
        self._chk(self._L.mf_end_frame(self._h, timestamp))

    # the per-model loops of processFrame over this context's list (mf_track_models / mf_fuse_models / mf_predict_models): one batched
    # Gauss-Newton loop, one launch per surfel pass for all object models.  firstModel = 1: models[0] is a background stand-in.
    def trackModels(self, firstModel: int = 0, trackAllModels: bool = True):
        """the tracking loop, Core/MaskFusion.cpp:247-276"""
        self._chk(self._L.mf_track_models(self._h, firstModel, int(bool(trackAllModels))))

    def fuseModels(self, firstModel: int = 0, weightMultiplier: float = 1.0, spawnedModel: int = -1):
        """:335-374 object parameters and the spawn-frame pass of models[spawnedModel], then the fusion loop :539-565"""
        self._chk(self._L.mf_fuse_models(self._h, firstModel, float(weightMultiplier), spawnedModel))

    def predictModels(self, firstModel: int = 0, timestamp: int = 0):
        """predict() :569 + tick++ / pose log / age++ (the end of a frame sequenced by the caller; replaces endFrame)"""
        self._chk(self._L.mf_predict_models(self._h, firstModel, timestamp))

    def modelIDs(self):
        """ids of the model list in list order (host state: does not wait for the device, unlike Model.getID)"""
        ids = (C.c_int32 * 256)()
        n = C.c_int32(0)
        self._chk(self._L.mf_get_model_ids(self._h, ids, 256, C.byref(n)))
        return [int(ids[i]) for i in range(n.value)]

    def modelsStateDevice(self, d_out16: int, capacity: int):
        """modelStateDevice for the whole list: 16 floats per model into one device buffer"""
        self._chk(self._L.mf_models_state_dev(self._h, d_out16, capacity))

    def setTrackableClassIds(self, ids):
        a = np.ascontiguousarray(list(ids), np.int32)
        self._chk(self._L.mf_set_trackable_class_ids(self._h, a.ctypes.data if len(a) else None, len(a)))

    def predict(self):
        self._chk(self._L.mf_predict(self._h))

    def preallocateModels(self, count: int):
        self._chk(self._L.mf_preallocate_models(self._h, count))

    # -- inactive models and their re-detection (MaskFusion.h:311,398-399: inactiveModels, redetectModels; shipped empty upstream) --------
    REDETECT_MIN_AGE = 25                  # frames: the age at which the object confidence ramp min(4.5, age / 25) reaches 1 (MaskFusion.cpp:369-374)

    def setEnableRedetection(self, on: bool, merge: bool = False):
        """MaskFusion::enableRedetection (default off): processFrame calls redetectModels(merge=merge) after every frame.  The maps to
        recognise come from setParam("keepInactiveModels", 1), which this does not set."""
        self._redetect = bool(on)
        self._redetect_merge = bool(merge)

    def inactiveModels(self) -> list:
        """the kept maps of dropped models, in the order of the drops: one InactiveInfo (id, class_id, surfels, age, confidence_threshold,
        tick, pose: 16 floats column-major) each"""
        n = C.c_int32(0)
        self._chk(self._L.mf_inactive_count(self._h, C.byref(n)))
        out = []
        for k in range(n.value):
            info = InactiveInfo()
            self._chk(self._L.mf_inactive_info(self._h, k, C.byref(info)))
            out.append(info)
        return out

    def inactiveMap(self, k: int) -> np.ndarray:
        """the archive of inactive model k as Model.downloadMap lays a map out: (surfels, 12) float32"""
        cnt = C.c_uint32(0)
        self._chk(self._L.mf_inactive_download_map(self._h, k, None, 0, C.byref(cnt)))
        out = np.zeros((max(cnt.value, 1), 12), np.float32)
        self._chk(self._L.mf_inactive_download_map(self._h, k, out.ctypes.data, cnt.value, C.byref(cnt)))
        return out[:cnt.value]

    def reactivateModel(self, k: int, pose=None):
        """mf_reactivate_model: inactive model k returns to the end of the model list under its old id, with its archived map, non-static, at
        `pose` (4 x 4, Model.overridePose's argument) or at its archived pose"""
        p = None if pose is None else np.ascontiguousarray(np.asarray(pose, np.float32).T.reshape(16))
        self._chk(self._L.mf_reactivate_model(self._h, k, p.ctypes.data if p is not None else None))

    def discardInactive(self, k: int):
        self._chk(self._L.mf_inactive_discard(self._h, k))

    def redetectModels(self, min_age: int | None = None, merge: bool = False, **match) -> list:
        """MaskFusion::redetectModels.  For every object model whose age is exactly `min_age` (REDETECT_MIN_AGE by default: a new model is
        looked at once, when its map has had that many frames to grow) and every inactive model of the same class, in list order,
        maskfusion_amd.redetect.match_model(new map, archived map, **match).  On the first acceptance the archived model is reactivated in the
        new one's place and the new one is dropped without being kept.  Returns the merged pairs [(new id, old id), ...].
        merge=True: the new model's map is not lost with it but merged into the reactivated map (Model.mergeMap with match_model's T, new ->
        old, radius voxel / 2 -- the acceptance test's -- and the default normal gate): what the camera saw of the object during its second
        visit stays.  The default drops it.

        The pose.  A model's pose P (Model.getPose / overridePose) takes camera coordinates to the model's: a surfel n of the map is seen at
        P^-1 n.  match_model's T takes the new map onto the old one, o = T n.  The returning object must stay where the camera sees the new
        one, P_old^-1 o = P_new^-1 n for every n, so P_old^-1 T = P_new^-1:  P_old = T P_new.  (With poses written the other way round, model to
        camera, Q = P^-1, the same statement reads Q_old = Q_new T^-1.)"""
        from . import redetect
        min_age = self.REDETECT_MIN_AGE if min_age is None else int(min_age)
        merged = []
        if not self.inactiveModels():       # (host state: a run without archived models pays no synchronisation for the question)
            return merged
        i = 1
        while i < len(self.modelIDs()):
            m = Model(self, i)
            info = m.info()
            done = False
            if info.age == min_age and all(info.id != old_id for _, old_id in merged):      # (not a model this call brought back)
                new_map = None
                for k, old in enumerate(self.inactiveModels()):
                    if old.class_id != info.class_id:
                        continue
                    new_map = m.downloadMap() if new_map is None else new_map
                    r = redetect.match_model(new_map, self.inactiveMap(k), **match)
                    if not r["accepted"]:
                        continue
                    pose = r["T"] @ m.getPose()
                    keep = self.getParam("keepInactiveModels")
                    self.setParam("keepInactiveModels", 0)          # the new model is dropped for good
                    try:
                        self._chk(self._L.mf_drop_model(self._h, i))
                    finally:
                        self.setParam("keepInactiveModels", keep)
                    self.reactivateModel(k, pose)
                    if merge:                                       # (the reactivated model stands at the end of the list)
                        Model(self, len(self.modelIDs()) - 1).mergeMap(new_map, T=r["T"], radius=r["voxel"] / 2.0)
                    merged.append((int(info.id), int(old.id)))
                    done = True
                    break
            if not done:
                i += 1
        return merged

    # -- exports (Core/MaskFusion.h:282-284) --------------------------------------------------------
    def savePly(self, exportDir: str):
        self._chk(self._L.mf_save_ply(self._h, exportDir.encode()))

    def saveMesh(self, exportDir: str, voxel: float, support: float | None = None, min_neighbours: int = 3):
        """mesh-<id>.ply per model, beside savePly's cloud-<id>.ply: the surfels savePly writes (confidence above the model's threshold, from
        mf_download_map), their normal (offset 8, negated as savePly negates it: it then faces the camera that saw the surfel) and their
        colour decoded on the host, meshed on the GPU (maskfusion_amd.mesh.mesh_cloud, DESIGN.md "Surfel meshing"; model frame).  A model
        without such surfels gets a file with no vertices.  Returns the paths."""
        from . import mesh as _mesh
        paths = []
        for m in self.getModels():
            rec = m.downloadMap()
            rec = rec[rec[:, 3] > m.getConfidenceThreshold()]
            col = rec[:, 4].astype(np.int64)
            rgb = np.stack([col >> 16 & 0xFF, col >> 8 & 0xFF, col & 0xFF], 1).astype(np.float32)
            v, n, c, t = _mesh.mesh_cloud(rec[:, :3], -rec[:, 8:11], rgb, voxel=voxel, support=support, min_neighbours=min_neighbours)
            paths.append(f"{exportDir}mesh-{m.getID()}.ply")
            _mesh.write_mesh_ply(paths[-1], v, n, c, t)
        return paths

    def exportPoses(self, exportDir: str):
        self._chk(self._L.mf_export_poses(self._h, exportDir.encode()))

    def getPoseLog(self, model: int = 0):
        """(timestamps int64[n], poses float32[n, 7] = tx ty tz qx qy qz qw), Model::getPoseLog."""
        n = C.c_uint32(0)
        self._chk(self._L.mf_get_pose_log(self._h, model, None, None, 0, C.byref(n)))
        ts = np.zeros(n.value, np.int64)
        p = np.zeros((n.value, 7), np.float32)
        if n.value:
            self._chk(self._L.mf_get_pose_log(self._h, model, ts.ctypes.data, p.ctypes.data, n.value, C.byref(n)))
        return ts, p

    # -- getters ----------------------------------------------------------------------------------
    def getTick(self) -> int:
        t = C.c_int32(0)
        self._chk(self._L.mf_get_tick(self._h, C.byref(t)))
        return t.value

    def setTick(self, tick: int):
        self._chk(self._L.mf_set_tick(self._h, int(tick)))

    def getBackgroundModel(self) -> Model:
        return Model(self, 0)

    def getModels(self):
        n = C.c_int32(0)
        self._chk(self._L.mf_num_models(self._h, C.byref(n)))
        return [Model(self, i) for i in range(n.value)]

    def getCurrPose(self) -> np.ndarray:
        return self.getBackgroundModel().getPose()

    def downloadSegmentation(self) -> np.ndarray:
        """SegmentationResult::fullSegmentation of the last frame (model id per pixel, 255 = ignored)."""
        out = np.zeros((self.height, self.width), np.uint8)
        self._chk(self._L.mf_download_segmentation(self._h, out.ctypes.data))
        return out

    def exportSegmentation(self, path: str):
        """the exportSegmentation branch of processFrame (MaskFusion.cpp:299-303): label image, 255 zeroed, as an 8-bit PNG"""
        self._chk(self._L.mf_export_segmentation_png(self._h, path.encode()))

    def getLastFillIn(self) -> bool:
        u = C.c_int32(0)
        self._chk(self._L.mf_get_last_fillin(self._h, C.byref(u)))
        return bool(u.value)

    # -- setters (MaskFusion.h:132-182) --------------------------------------------------------------
    def setParam(self, key: str, value: float):
        self._chk(self._L.mf_set_param(self._h, key.encode(), float(value)))

    def getParam(self, key: str) -> float:
        v = C.c_double(0)
        self._chk(self._L.mf_get_param(self._h, key.encode(), C.byref(v)))
        return v.value

    def setDepthCutoff(self, v): self.setParam("depthCutoff", v)
    def setIcpWeight(self, v): self.setParam("icpWeight", v)
    def setConfidenceThreshold(self, v): self.setParam("confidenceThreshold", v)
    def setOutlierCoefficient(self, v): self.setParam("outlierCoefficient", v)
    def setFastOdom(self, v): self.setParam("fastOdom", int(v))
    def setSo3(self, v): self.setParam("so3", int(v))
    def setFrameToFrameRGB(self, v): self.setParam("frameToFrameRGB", int(v))   # Core/MaskFusion.cpp:910
    def setRgbOnly(self, v): self.setParam("rgbOnly", int(v))

    def trackStats(self, model: int = 0) -> dict:
        """Statistics of the last tracking step (RGBDOdometry.h:68-75)."""
        out = np.zeros(8, np.float32)
        self._chk(self._L.mf_get_track_stats(self._h, model, out.ctypes.data))
        keys = ("lastICPError", "lastICPCount", "lastRGBError", "lastRGBCount", "lastSO3Error", "lastSO3Count", "so3Iterations",
                "rejected")
        return dict(zip(keys, out.tolist()))
    def gnIllIterations(self, model: int = 0) -> int:
        """Gauss-Newton iterations of the last geometric tracking step whose system was outside the solver's stated domain (finding F4)"""
        n = C.c_int32(0)
        self._chk(self._L.mf_get_gn_condition(self._h, model, C.byref(n)))
        return n.value

    def setPyramid(self, v): self.setParam("pyramid", int(v))
    def setEnableMultipleModels(self, v): self.setParam("enableMultipleModels", int(v))

    def enableTimings(self, on=True):
        self.setParam("timings", 1 if on else 0)

    def timings(self) -> dict:
        t = np.zeros(MF_N_TIMINGS, np.float32)
        self._chk(self._L.mf_get_timings(self._h, t.ctypes.data))
        return dict(zip(TIMING_LABELS, t.tolist()))

    def passTimings(self) -> dict:
        """GPU milliseconds of the surfel passes of the last frame, pass by pass (setParam("passTimings", 1); labels: maskfusion_amd.h MF_PASS_*)"""
        t = np.zeros(MF_N_PASSES, np.float32)
        self._chk(self._L.mf_get_pass_timings(self._h, t.ctypes.data))
        return dict(zip(PASS_LABELS, t.tolist()))

    def stream(self) -> int:
        return int(self._L.mf_get_stream(self._h) or 0)

    def inputStream(self) -> int:
        """hipStream_t on which frames handed to processFrameDevice are first read (see include/maskfusion_amd.h)."""
        return int(self._L.mf_get_input_stream(self._h) or 0)

    # -- differential-test taps ----------------------------------------------------------------------
    # -- headless rendering (Model::renderPointCloud as MainController::drawScene draws the models; include/maskfusion_amd.h) ----------
    def defaultRenderView(self, width: int = 1280, height: int = 980, icl: bool = False) -> RenderView:
        """The GUI's follow-pose view: the current camera 0.2 m back along its axis, fx = fy = 420, centred principal point, near 0.1, far 1000"""
        v = RenderView()
        self._chk(self._L.mf_default_render_view(self._h, int(width), int(height), int(bool(icl)), C.byref(v)))
        return v

    def sensorRenderView(self) -> RenderView:
        """The view of the frame just processed (mf_sensor_render_view): the context's image size and intrinsics, the current camera pose,
        near 0.01, far 1000, both colour types 2, cleared to opaque black -- what maskfusion_amd.eval.ViewScorer compares with the frame"""
        v = RenderView()
        self._chk(self._L.mf_sensor_render_view(self._h, C.byref(v)))
        return v

    @staticmethod
    def defaultPalette() -> np.ndarray:
        """the library's own label palette, (n, 3) float32 RGB in [0, 1] (class ids index it modulo n)"""
        L, n = load(), C.c_int32(0)
        if L.mf_default_palette(None, 0, C.byref(n)) != 0:
            raise MFError("mf_default_palette failed")
        out = np.zeros((n.value, 3), np.float32)
        if L.mf_default_palette(out.ctypes.data, n.value, C.byref(n)) != 0:
            raise MFError("mf_default_palette failed")
        return out

    def renderView(self, view: RenderView | None = None, palette=None, depth: bool = False, models: bool = False):
        """Renders the maps from `view` (default: defaultRenderView()).  Returns the (H, W, 4) uint8 image, plus the (H, W) float32 camera z
        (0: nothing drawn) with depth=True and the (H, W) int32 model list index (-1: none) with models=True, in that order.
        palette: (n, 3) RGB for colour type 4 (None: the library's palette)."""
        if view is None:
            view = self.defaultRenderView()
        H, W = int(view.height), int(view.width)
        rgba = np.zeros((max(H, 1), max(W, 1), 4), np.uint8)
        dep = np.zeros((max(H, 1), max(W, 1)), np.float32) if depth else None
        mod = np.zeros((max(H, 1), max(W, 1)), np.int32) if models else None
        if palette is None:
            pal_ptr, n_pal = None, 0
        else:
            pal = np.ascontiguousarray(np.asarray(palette, np.float32).reshape(-1, 3))
            n_pal = len(pal)
            if n_pal == 0:
                pal = np.zeros((1, 3), np.float32)   # an empty palette: a valid pointer with n = 0 (the library refuses it for colour type 4)
            pal_ptr = pal.ctypes.data
        self._chk(self._L.mf_render_view(self._h, C.byref(view), pal_ptr, n_pal, rgba.ctypes.data,
                                         dep.ctypes.data if dep is not None else None, mod.ctypes.data if mod is not None else None))
        out = [rgba]
        if depth:
            out.append(dep)
        if models:
            out.append(mod)
        return out[0] if len(out) == 1 else tuple(out)

    def renderViewDevice(self, view: RenderView, d_rgba: int, d_depth: int = 0, d_model: int = 0, palette=None):
        """mf_render_view_dev: device outputs (raw pointers), enqueued on stream() without waiting"""
        pal_ptr, n_pal, keep = None, 0, None
        if palette is not None:
            keep = np.ascontiguousarray(np.asarray(palette, np.float32).reshape(-1, 3))
            pal_ptr, n_pal = keep.ctypes.data, len(keep)
        self._chk(self._L.mf_render_view_dev(self._h, C.byref(view), pal_ptr, n_pal, d_rgba, d_depth or None, d_model or None))

    # -- run evaluation (include/maskfusion_amd.h: mf_model_cloud_nn_dev) ------------------------------------------------------------
    def modelCloudNN(self, model: int, points, radius: float, transform=None, confThreshold=None):
        """Nearest surfel of `model` within `radius` of every point, read from the live map without downloading it.  points: (n, 3 or more)
        float32, a numpy array or a torch tensor on the library's device; transform: 4 x 4 mapping the points into the model's frame;
        confThreshold: the surfels taken (confidence > it; None: the model's own threshold, what savePly writes).  Returns (dist, idx) of the
        kind it was given: dist float32 (+inf: none), idx int32 indexing Model.downloadMap() (-1: none)."""
        import torch
        from .lib import torch_device
        as_numpy = not isinstance(points, torch.Tensor)
        q = torch.as_tensor(np.ascontiguousarray(points, np.float32)) if as_numpy else points
        if q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] < 3:
            raise MFError("modelCloudNN: points must be (n, >= 3) float32")
        q = q.to(torch_device()).contiguous()
        n = int(q.shape[0])
        dist = torch.empty(max(n, 1), dtype=torch.float32, device=q.device)
        idx = torch.empty(max(n, 1), dtype=torch.int32, device=q.device)
        thr = Model(self, model).getConfidenceThreshold() if confThreshold is None else float(confThreshold)
        T = None if transform is None else np.ascontiguousarray(np.asarray(transform, np.float32).T.reshape(16))
        if q.device.type == "cuda":
            # the call runs on the context's own (non-blocking) stream: torch's pending work on the queries, and on the memory the caching
            # allocator handed out for dist / idx, must be done first.  The call waits for its stream before returning, so the outputs are
            # complete for any stream afterwards.
            torch.cuda.current_stream(q.device).synchronize()
        self._chk(self._L.mf_model_cloud_nn_dev(self._h, int(model), thr, q.data_ptr() if n else None, int(q.shape[1]), n,
                                                T.ctypes.data if T is not None else None, float(radius), dist.data_ptr(), idx.data_ptr()))
        dist, idx = dist[:n], idx[:n]
        if as_numpy:
            return dist.cpu().numpy(), idx.cpu().numpy()
        return dist, idx

    def debugRead(self, what: str, model: int = 0, count: int | None = None) -> np.ndarray:
        """count: number of records for the variable-length taps (cand_op, cand_rec, clean_flags, clean_newconf)"""
        W, H = self.width, self.height
        shapes = {"depthF": ((H, W), np.float32), "pred_vertex": ((H, W, 4), np.float32),
                  "pred_normal": ((H, W, 4), np.float32), "pred_image": ((H, W, 4), np.uint8), "pred_time": ((H, W), np.uint16),
                  "index": ((H, W), np.int32), "index_vc": ((H, W, 4), np.float32), "index_nr": ((H, W, 4), np.float32),
                  "index_ct": ((H, W, 4), np.float32), "index_packed": ((W, H, 2, 4), np.float32),  "icp_log": ((19, 32), np.float32), "gn_trace": ((20, 64), np.float64),
                  "icp_prof": ((19, 16), np.uint64), "splat_prof": ((((H + 15) // 16) * ((W + 15) // 16), 8), np.uint64),
                  "edge_map": ((H, W), np.float32),
                  "edge_binary": ((H, W), np.uint8), "projected_ids": ((H, W), np.uint8)}
        for i in range(3):      # the frame's intensity pyramid and its derivative / gate images (photometric term, SO(3))
            shapes.update({f"gray{i}": ((H >> i, W >> i), np.uint8), f"dIdx{i}": ((H >> i, W >> i), np.int16), f"dIdy{i}": ((H >> i, W >> i), np.int16),
                           f"rgb_gate{i}": ((H >> i, W >> i), np.uint8)})
        if count is not None:
            shapes.update({"cand_op": ((count,), np.uint8), "cand_rec": ((count, 12), np.float32),
                           "clean_flags": ((count,), np.uint8), "clean_newconf": ((count,), np.float32)})
        for pre in ("vmap_g", "nmap_g", "vmap", "nmap"):
            for i in range(3):
                shapes[f"{pre}{i}"] = ((3, H >> i, W >> i), np.float32)
        if what == "index_packed" and int(self.getParam("indexPackedTexelBytes")) == 16:
            shapes[what] = ((W, H, 4), np.float32)      # the last frame wrote 16-byte taps ("cleanTap16"): {x, y, z', initTime}
        shape, dt = shapes[what]
        out = np.zeros(shape, dt)
        self._chk(self._L.mf_debug_read_model(self._h, model, what.encode(), out.ctypes.data, out.nbytes))
        return out
