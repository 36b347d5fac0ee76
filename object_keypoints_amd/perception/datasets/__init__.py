"""The target half of the reference's SceneDataset (perception/datasets/video.py:50-263): labelled 3D key points and camera poses ->
labels and target maps, on the device.  No video, h5py or augmentation: frames come from the caller."""
import numpy as np
import torch

from object_keypoints_amd import ops
from object_keypoints_amd.ops import OkpError


class SceneTargets:
    """keypoint_config: the configuration file's dict (or its 'keypoint_config' list); camera: a camera_utils camera of the RAW frames;
    world_points: the '3d_points' of keypoints.json ([n_objects * (nk - 1), >= 3], object-major).  The per-object centre is inserted as
    the mean of the object's key points, in front of them (SceneDataset._init_points, video.py:108-125)."""

    def __init__(self, keypoint_config, camera, world_points, raw_size=(720, 1280), device=None):
        cfg = keypoint_config['keypoint_config'] if isinstance(keypoint_config, dict) else keypoint_config
        self.keypoint_config = [1] + [int(c) for c in cfg]
        self.n_keypoints = sum(self.keypoint_config)
        self.keypoint_maps = len(self.keypoint_config)
        points = np.asarray(world_points, dtype=np.float64)
        real = self.n_keypoints - 1
        if points.ndim != 2 or points.shape[1] < 3 or points.shape[0] == 0 or points.shape[0] % real:
            raise OkpError(f"world_points must be [n_objects * {real}, 3]: wrong number of keypoints {points.shape}")
        self.n_objects = points.shape[0] // real
        ops.check_type_count(self.keypoint_config, self.n_objects)
        self.world_points = np.zeros((self.n_keypoints * self.n_objects, 3))
        for i in range(self.n_objects):
            obj = points[i * real:(i + 1) * real, :3]
            self.world_points[i * self.n_keypoints] = obj.mean(axis=0)
            self.world_points[i * self.n_keypoints + 1:(i + 1) * self.n_keypoints] = obj
        self.camera = camera
        self.cam = camera.okp()
        self.scale, self.crop_x, self.crop_y = ops.raw_to_input(raw_size)
        self.device = device
        self._world_dev = None

    def truth_points(self):
        """world_points as [n_objects, nk, 3], row 0 of every object its centre: what perception.evaluation.DeviceResults takes."""
        return self.world_points.reshape(self.n_objects, self.n_keypoints, 3).copy()

    def labels(self, T_WC):
        """Camera poses T_WC [N,4,4] (NumPy or tensor) -> {"points": [N, n_objects * nk, 3] fp64, "n_obj": [N] int32} on the device."""
        dev = torch.device(self.device if self.device is not None else "cuda")
        T = torch.as_tensor(np.asarray(T_WC, dtype=np.float64) if not isinstance(T_WC, torch.Tensor) else T_WC)
        if T.dtype != torch.float64 or T.dim() != 3 or tuple(T.shape[1:]) != (4, 4):
            raise OkpError("T_WC must be float64 [N, 4, 4]")
        if not torch.cuda.is_available():
            raise OkpError("SceneTargets.labels needs a device: the HIP path has no CPU fallback")
        T = T.to(dev).contiguous()
        if self._world_dev is None or self._world_dev.device != T.device:
            self._world_dev = torch.from_numpy(self.world_points).to(T.device)
        pts = ops.project_labels(self.cam, self._world_dev, T, self.scale, (self.crop_x, self.crop_y))
        return {"points": pts, "n_obj": torch.full((T.shape[0],), self.n_objects, dtype=torch.int32, device=T.device)}

    def render(self, labels):
        """labels -> the dense (heat [N,K,64,64], depth [N,K,64,64], centers [N,K-1,2,64,64]) the reference's dataset yields."""
        return ops.render_targets(labels["points"], labels["n_obj"], self.keypoint_config)
