"""``streamingflow`` — the whole model, from camera images and point clouds, wired from the MI355X-native parts.

Mirrors ``streamingflow.forward`` (streamingflow/models/streamingflow.py:208-269) with the reference's
attribute names (``temporal_model``, ``encoders.lidar.{voxelize,backbone}``, ``temporal_model_lidar``,
``future_prediction_ode``, ``decoder``, ``bev_resolution`` / ``bev_start_position`` / ``bev_dimension``,
``frustum``), so a released ``model.*`` checkpoint slice loads with ``strict=False``.  The image ``Encoder``
(streamingflow/models/encoder.py) is models/encoder.py (the neck) over models/efficientnet.py (the EfficientNet trunk, restated:
``efficientnet_pytorch`` is not needed): pass ``encoder=camera_encoder(cfg)`` — ``Encoder(cfg.MODEL.ENCODER, D,
backbone=EfficientNetTrunk("b4"))`` with the two keys ``default_cfg`` leaves out — or assign it to ``self.encoder``: its
outputs then reach the lift in the layouts the lift reads.  The default stays ``encoder=None``; or assign any module returning
``(features [b*n, C, fH, fW], depth_logits [b*n, D, fH, fW])``, or pass that pair in place of ``image``.

Camera:  (features, depth logits, rig) -> LiftSplat.lift_splat -> + ego-pose channels -> TemporalModel
LiDAR:   point clouds -> hard voxelisation + mean -> SparseEncoder -> TemporalModel
both  -> FuturePredictionODE -> Decoder.
"""
from types import SimpleNamespace as NS

import torch
import torch.nn as nn

from .decoder import Decoder
from .future_prediction_ode import FuturePredictionODE
from .lift_splat import LiftSplat
from .planning import Planning
from .sparse_encoder import SparseEncoder
from .temporal_model import TemporalModel
from ..voxelize import Voxelization, voxelize, voxelize_static

# the LiDAR encoder configuration hard-coded at streamingflow.py:111
LIDAR_ENCODER = {"voxelize": {"max_num_points": 10, "point_cloud_range": [-50.0, -50.0, -5.0, 50.0, 50.0, 3.0],
                              "voxel_size": [0.0625, 0.0625, 0.2], "max_voxels": [120000, 160000]},
                 "backbone": {"in_channels": 5, "sparse_shape": [1600, 1600, 41], "output_channels": 128,
                              "order": ["conv", "norm", "act"],
                              "encoder_channels": [[16, 16, 32], [32, 32, 64], [64, 64, 128], [128, 128]],
                              "encoder_paddings": [[0, 0, 1], [0, 0, 1], [0, 0, [1, 1, 0]], [0, 0]], "block_type": "basicblock"}}


def default_cfg(**over):
    """The configuration keys this stage reads, with the reference's defaults (streamingflow/config.py)."""
    cfg = NS(TIME_RECEPTIVE_FIELD=3, N_FUTURE_FRAMES=4,
             IMAGE=NS(FINAL_DIM=(224, 480), ORIGINAL_HEIGHT=900, ORIGINAL_WIDTH=1600, RESIZE_SCALE=0.3, TOP_CROP=46),
             LIFT=NS(X_BOUND=[-50.0, 50.0, 0.5], Y_BOUND=[-50.0, 50.0, 0.5], Z_BOUND=[-10.0, 10.0, 20.0], D_BOUND=[2.0, 50.0, 1.0],
                     DISCOUNT=0.5),
             MODEL=NS(ENCODER=NS(DOWNSAMPLE=8, OUT_CHANNELS=64),
                      MODALITY=NS(USE_CAMERA=True, USE_LIDAR=True),
                      TEMPORAL_MODEL=NS(NAME="temporal_block", START_OUT_CHANNELS=64, EXTRA_IN_CHANNELS=0, INBETWEEN_LAYERS=0,
                                        PYRAMID_POOLING=True, INPUT_EGOPOSE=True),
                      DISTRIBUTION=NS(LATENT_DIM=64),
                      FUTURE_PRED=NS(N_GRU_BLOCKS=2, N_RES_LAYERS=1, MIXTURE=True, DELTA_T=0.05, USE_VARIABLE_ODE_STEP=True),
                      IMPUTE=True, SOLVER="euler", SMALL_ENCODER=NS(FILTER_SIZE=64, SKIPCO=False)),
             SEMANTIC_SEG=NS(VEHICLE=NS(WEIGHTS=[1.0, 2.0]), PEDESTRIAN=NS(ENABLED=False), HDMAP=NS(ENABLED=False, ELEMENTS=["lane_divider", "drivable_area"])),
             INSTANCE_SEG=NS(ENABLED=True), INSTANCE_FLOW=NS(ENABLED=True),
             # the planner is off unless asked for; GRU_STATE_SIZE 256 is what reduce_channel makes of a [64, 28, 60] front-camera map
             PLANNING=NS(ENABLED=False, GRU_STATE_SIZE=256, SAMPLE_NUM=600, COMMAND=["LEFT", "FORWARD", "RIGHT"]),
             EGO=NS(WIDTH=1.85, HEIGHT=4.084),
             COST_FUNCTION=NS(SAFETY=0.1, LAMBDA=1.0, HEADWAY=1.0, LRDIVIDER=10.0, COMFORT=0.1, PROGRESS=0.5, VOLUME=100.0),
             LIDAR_ENCODER=LIDAR_ENCODER)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def camera_encoder(cfg, version="b4", **trunk_kw):
    """The reference's image ``Encoder`` for ``cfg`` on the device: the neck over ``EfficientNetTrunk(version)`` — pass it as
    ``streamingflow(cfg, encoder=camera_encoder(cfg))``.  ``cfg.MODEL.ENCODER`` gives DOWNSAMPLE and OUT_CHANNELS; NAME and
    USE_DEPTH_DISTRIBUTION, which ``Encoder`` reads and ``default_cfg`` does not carry, are taken from it when present and otherwise
    supplied here (``efficientnet-<version>``, True); D is the number of depth bins of ``cfg.LIFT.D_BOUND``.  ``trunk_kw``: ``image_size``."""
    from .efficientnet import EfficientNetTrunk
    from .encoder import Encoder
    e = cfg.MODEL.ENCODER
    name = getattr(e, "NAME", "efficientnet-" + version)
    enc_cfg = NS(NAME=name, OUT_CHANNELS=e.OUT_CHANNELS, DOWNSAMPLE=e.DOWNSAMPLE, USE_DEPTH_DISTRIBUTION=getattr(e, "USE_DEPTH_DISTRIBUTION", True))
    D = len(torch.arange(*cfg.LIFT.D_BOUND, dtype=torch.float))
    return Encoder(enc_cfg, D, backbone=EfficientNetTrunk(name.split("-")[1], e.DOWNSAMPLE, **trunk_kw))


class streamingflow(nn.Module):
    def __init__(self, cfg, encoder=None, frontend=None):
        super().__init__()
        self.cfg = cfg
        # image front end: None unless given (or assigned later): ImageFrontend.from_cfg(cfg) takes raw uint8 frames and raw intrinsics
        self.image_frontend = frontend
        self.lift = LiftSplat.from_cfg(cfg)
        # opt-in, the camera's counterpart of `static_lidar`: the lift takes the rig's affines from the device kernel (LiftSplat.device_affines),
        # no host read, so `forward` can be recorded into a graph from raw intrinsics; `lift.check_rig()` reports a bad camera
        self.static_camera = False
        # the reference keeps these on the top-level module (streamingflow.py:31-33, :41)
        self.bev_resolution, self.bev_start_position, self.bev_dimension = self.lift.bev_resolution, self.lift.bev_start_position, self.lift.bev_dimension
        self.frustum = self.lift.frustum
        self.encoder_out_channels = cfg.MODEL.ENCODER.OUT_CHANNELS
        self.use_lidar, self.use_camera = cfg.MODEL.MODALITY.USE_LIDAR, cfg.MODEL.MODALITY.USE_CAMERA
        self.receptive_field, self.n_future = cfg.TIME_RECEPTIVE_FIELD, cfg.N_FUTURE_FRAMES
        self.latent_dim = cfg.MODEL.DISTRIBUTION.LATENT_DIM
        self.planning_enabled = bool(getattr(getattr(cfg, "PLANNING", None), "ENABLED", False))
        self.bev_size = (int(self.bev_dimension[0]), int(self.bev_dimension[1]))
        # image encoder: None unless given (or assigned later): camera_encoder(cfg) builds the reference's (neck + EfficientNet trunk)
        self.encoder = encoder
        tm = cfg.MODEL.TEMPORAL_MODEL
        if tm.NAME != "temporal_block":
            raise NotImplementedError("TEMPORAL_MODEL.NAME == 'temporal_block' only")
        kw = dict(input_shape=self.bev_size, start_out_channels=tm.START_OUT_CHANNELS, extra_in_channels=tm.EXTRA_IN_CHANNELS,
                  n_spatial_layers_between_temporal_layers=tm.INBETWEEN_LAYERS, use_pyramid_pooling=tm.PYRAMID_POOLING)
        if self.use_camera:
            self.temporal_model = TemporalModel(self.encoder_out_channels + (6 if tm.INPUT_EGOPOSE else 0), self.receptive_field, **kw)
        self.future_pred_in_channels = tm.START_OUT_CHANNELS
        if self.n_future > 0:
            fp = cfg.MODEL.FUTURE_PRED
            self.future_prediction_ode = FuturePredictionODE(in_channels=self.future_pred_in_channels, latent_dim=self.latent_dim,
                                                             n_future=self.n_future, cfg=cfg, mixture=fp.MIXTURE, n_gru_blocks=fp.N_GRU_BLOCKS,
                                                             n_res_layers=fp.N_RES_LAYERS, delta_t=fp.DELTA_T)
        self.decoder = Decoder(in_channels=self.future_pred_in_channels, n_classes=len(cfg.SEMANTIC_SEG.VEHICLE.WEIGHTS),
                               n_present=self.receptive_field, n_hdmap=len(cfg.SEMANTIC_SEG.HDMAP.ELEMENTS),
                               predict_gate={"perceive_hdmap": cfg.SEMANTIC_SEG.HDMAP.ENABLED,
                                             "predict_pedestrian": cfg.SEMANTIC_SEG.PEDESTRIAN.ENABLED,
                                             "predict_instance": cfg.INSTANCE_SEG.ENABLED,
                                             "predict_future_flow": cfg.INSTANCE_FLOW.ENABLED, "planning": self.planning_enabled})
        if self.planning_enabled:
            self.planning = Planning(cfg, self.encoder_out_channels, 6, gru_state_size=cfg.PLANNING.GRU_STATE_SIZE)
        if self.use_lidar:
            enc = getattr(cfg, "LIDAR_ENCODER", LIDAR_ENCODER)
            self.encoders = nn.ModuleDict({"lidar": nn.ModuleDict({
                "voxelize": Voxelization(**{k: (tuple(v) if k == "max_voxels" else v) for k, v in enc["voxelize"].items()}),
                "backbone": SparseEncoder(**enc["backbone"])})})
            self.voxelize_reduce = True
            # opt-in: the LiDAR branch sized by capacities fixed in advance (max_voxels per cloud, SparseEncoder.default_capacities or
            # `lidar_capacities`), no host read, so `forward` can be recorded into a graph; the device counts of the last call stay in
            # `lidar_site_counts` for SparseEncoder.check_static
            self.static_lidar = False
            self.lidar_capacities = None
            self.lidar_site_counts = None
            self.lidar_channels = enc["backbone"]["output_channels"] * self._lidar_depth(enc["backbone"])
            self.temporal_model_lidar = TemporalModel(self.lidar_channels, self.receptive_field, **kw)

    @staticmethod
    def _lidar_depth(b):
        z = b["sparse_shape"][2]
        pads = b["encoder_paddings"]
        for i in range(len(b["encoder_channels"]) - 1):
            p = pads[i][-1]
            pz = p[2] if isinstance(p, (list, tuple)) else p
            z = (z + 2 * pz - 3) // 2 + 1
        return (z - 3) // 2 + 1                       # conv_out: kernel (1,1,3), stride (1,1,2)

    # ---- streamingflow.py:170-206 -------------------------------------------------------------------
    def voxelize(self, points):
        return voxelize(points, self.encoders["lidar"]["voxelize"], self.voxelize_reduce)

    def extract_lidar_features(self, x):
        if self.static_lidar:
            backbone = self.encoders["lidar"]["backbone"]
            feats, coords, _ = voxelize_static(x, self.encoders["lidar"]["voxelize"], pad_to=backbone._cin_pad_width())
            feature, self.lidar_site_counts = backbone.forward_static(feats, coords, len(x), self.lidar_capacities)
            return feature
        feats, coords, sizes = self.voxelize(x)
        return self.encoders["lidar"]["backbone"](feats, coords, len(x))

    def calculate_birds_eye_view_features(self, image, intrinsics, extrinsics, future_egomotion):
        """streamingflow.py:430-448 minus the image backbone: ``image`` is (features [b,s,n,C,fH,fW],
        depth logits [b,s,n,D,fH,fW]) or, with ``self.encoder`` set, the images [b,s,n,3,H,W].  The third result is the planner's
        ``cam_front``: the features of camera 1 in the last (present) frame (``encoder_forward``, :294-303), None with planning off."""
        if isinstance(image, (tuple, list)):
            feat, depth = image
        else:
            if self.encoder is None:
                raise RuntimeError("no image backbone: set `.encoder` or pass (features, depth_logits) instead of images")
            b, s, n = image.shape[:3]
            flat = image.reshape(b * s * n, *image.shape[3:])
            if hasattr(self.encoder, "neck_nhwc"):
                # the neck's own layouts go straight to the lift: NHWC rays and planar probabilities, no transpose, no softmax launch
                rays, logits, prob = self.encoder.forward_nhwc(flat)
                D, (fH, fW) = logits.shape[1], self.frustum.shape[1:3]
                depth = logits.view(b, s, n, D, fH, fW)
                x = self.lift.lift_splat(None, depth, intrinsics, extrinsics, future_egomotion, rays_nhwc=rays, depth_prob=prob,
                                         device_affines=self.static_camera or None)
                cam_front = None
                if self.planning_enabled:      # only the front camera of the present frame goes back to NCHW
                    from .. import runtime
                    cam_front = runtime.to_nchw(rays.view(b, s, n, fH, fW, -1)[:, -1, 1].contiguous())
                return x, depth, cam_front
            feat, depth = self.encoder(flat)
            feat, depth = feat.view(b, s, n, *feat.shape[1:]), depth.view(b, s, n, *depth.shape[1:])
        x = self.lift.lift_splat(feat, depth, intrinsics, extrinsics, future_egomotion, device_affines=self.static_camera or None)
        cam_front = feat[:, -1, 1].contiguous() if self.planning_enabled else None
        return x, depth, cam_front

    def graphed(self, max_graphs=4):
        """``forward`` as one replayable graph (streamingflow_amd.model_graph.ModelGraphSession): ``session(*args)`` takes forward's
        arguments and returns forward's dict in the session's static outputs; at most ``max_graphs`` graphs are kept."""
        from ..model_graph import ModelGraphSession
        return ModelGraphSession(self, max_graphs=max_graphs)

    def forward(self, image, intrinsics, extrinsics, future_egomotion, padded_voxel_points=None, camera_timestamp=None, points=None,
                lidar_timestamp=None, target_timestamp=None):
        output = {}
        future_egomotion = future_egomotion[:, : self.receptive_field].contiguous()
        camera_states = lidar_states = states = None
        if self.use_lidar:
            pts = torch.stack(points).permute(1, 0, 2, 3)                       # B, T, num_point, C
            B, T, num_point, C = pts.shape
            pts = pts.contiguous().view(B * T, num_point, C).to(torch.float32)
            feature = self.extract_lidar_features([pts[i] for i in range(pts.shape[0])])
            _, C, H_det, W_det = feature.shape
            lidar_states = self.temporal_model_lidar(feature.view(B, T, C, H_det, W_det))
            states = lidar_states
        if self.use_camera:
            rf = self.receptive_field
            if isinstance(image, torch.Tensor) and image.dtype == torch.uint8:      # decoded frames [b, s, n, Hs, Ws, 3] and the cameras' own intrinsics
                if self.image_frontend is None:
                    raise RuntimeError("no image front end: set `.image_frontend` (ImageFrontend.from_cfg(cfg)) or pass float images instead of uint8 frames")
                image, intrinsics = self.image_frontend(image[:, :rf], intrinsics[:, :rf])      # only the frames the model reads
            img = tuple(t[:, :rf].contiguous() for t in image) if isinstance(image, (tuple, list)) else image[:, :rf].contiguous()
            x, depth, cam_front = self.calculate_birds_eye_view_features(img, intrinsics[:, :rf].contiguous(), extrinsics[:, :rf].contiguous(),
                                                                         future_egomotion)
            output = {**output, "depth_prediction": depth, "cam_front": cam_front}
            if self.cfg.MODEL.TEMPORAL_MODEL.INPUT_EGOPOSE:
                b, s, c = future_egomotion.shape
                h, w = x.shape[-2:]
                ego = future_egomotion.view(b, s, c, 1, 1).expand(b, s, c, h, w)
                ego = torch.cat([torch.zeros_like(ego[:, :1]), ego[:, : (rf - 1)]], dim=1)
                x = torch.cat([x, ego], dim=-3)
            camera_states = self.temporal_model(x)
            states = camera_states
        if self.n_future > 0:
            present_state = states[:, -1:].contiguous()
            states, _ = self.future_prediction_ode(present_state, camera_states, lidar_states, camera_timestamp, lidar_timestamp,
                                                   target_timestamp)
        bev_output = self.decoder(states)
        return {**output, **bev_output}
