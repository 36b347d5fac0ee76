"""KeypointLoss with the constructor and forward signature of the reference's perception/loss.py:5-48, as one device pass
(ops.keypoint_loss -> okp_keypoint_loss, csrc/okp_targets.hip): no boolean indexing, so no host synchronisation, and it can be
captured into a graph.  Forward only: there is no backward pass (training is out of scope)."""
import torch

from object_keypoints_amd import ops
from object_keypoints_amd.ops import OkpError


class KeypointLoss:
    def __init__(self, keypoint_config, depth_weight=10.0, center_weight=1.0, size_average=None, reduce=None, reduction='mean'):
        self.keypoint_config = [int(c) for c in keypoint_config]
        self.n_keypoint_maps = len(self.keypoint_config) + 1     # add one for the centre map (loss.py:9)
        self.type_count = [1] + self.keypoint_config
        ops.check_type_count(self.type_count)
        self.depth_weight = float(depth_weight)
        self.center_weight = float(center_weight)
        # the reference stores torch.mean / torch.sum under `reduce` and never uses it (loss.py:12-17): both give the same numbers
        if reduction not in ('mean', 'sum'):
            raise NotImplementedError(f"Unknown reduction method {reduction}, try 'mean' or 'sum'.")
        self.reduction = reduction

    @staticmethod
    def _tuple(r):
        return r["loss"], list(r["heat"].unbind(0)), list(r["depth"].unbind(0)), list(r["center"].unbind(0))

    def forward(self, p_heatmaps, gt_heatmaps, p_depth, gt_depth, p_centers, gt_centers):
        """The reference's 4-tuple (loss, heatmap_losses, depth_losses, center_losses) as fp64 device tensors; `self.last` keeps the whole
        result of ops.keypoint_loss (per-frame terms, mask counts)."""
        self.last = ops.keypoint_loss(p_heatmaps, p_depth, p_centers, self.type_count, targets=(gt_heatmaps, gt_depth, gt_centers),
                                      depth_weight=self.depth_weight, center_weight=self.center_weight)
        return self._tuple(self.last)

    __call__ = forward

    def from_labels(self, p_heatmaps, p_depth, p_centers, labels, first=0, state=None):
        """The fused form: `labels` = {"points": [N, max_obj * nk, 3] fp64, "n_obj": [N] int32} (SceneTargets.labels); the targets are
        rendered in registers and never stored.  first / state: a batch scored in chunks (ops.keypoint_loss); the 4-tuple is final after
        the chunk that ends the batch."""
        if not isinstance(labels, dict) or "points" not in labels or "n_obj" not in labels:
            raise OkpError('labels must be {"points": ..., "n_obj": ...} as SceneTargets.labels returns them')
        self.last = ops.keypoint_loss(p_heatmaps, p_depth, p_centers, self.type_count, labels=labels["points"], n_obj=labels["n_obj"],
                                      depth_weight=self.depth_weight, center_weight=self.center_weight, first=first,
                                      total=labels["points"].shape[0] if isinstance(labels["points"], torch.Tensor) else None, state=state)
        return self._tuple(self.last)
