"""ctypes binding of libvyolo.so (include/vyolo.h).  There is no CPU fallback: if the HIP
library is missing or fails to load, every entry point raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvyolo.so")

VY_MAX_TOPK = 1024
VY_CONV_EXACT_FP32, VY_CONV_SPLIT_BF16X3, VY_CONV_SPLIT_BF16X3_TRAIN = 0, 1, 2
VY_TAP_Z, VY_TAP_BN, VY_TAP_GRAD_PADDED, VY_TAP_INPUT_PADDED = 0, 1, 2, 3
VY_JOIN_MAX, VY_JOIN_MEAN = 0, 1
VY_HJOIN_MAX, VY_HJOIN_CONV = 0, 1
VY_VIDEO_TABLE_MAX = 512
VY_HIER_VIDEO_STEP_MAX = 64


class VyError(RuntimeError):
    """A libvyolo entry point returned a negative status."""

    def __init__(self, code, msg):
        super().__init__("libvyolo error %d: %s" % (code, msg))
        self.code = code


class ParamInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 96), ("kind", ctypes.c_int32), ("ndim", ctypes.c_int32),
                ("shape", ctypes.c_int32 * 4), ("size", ctypes.c_int64), ("offset", ctypes.c_int64),
                ("trainable", ctypes.c_int32), ("backbone", ctypes.c_int32)]


class ConvInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 96), ("cin", ctypes.c_int32), ("cout", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("pad", ctypes.c_int32), ("has_bn", ctypes.c_int32), ("sync_bn", ctypes.c_int32),
                ("residual", ctypes.c_int32), ("upsample", ctypes.c_int32), ("concat_offset", ctypes.c_int32),
                ("out_channels_total", ctypes.c_int32)]


class LaunchStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 64), ("ms", ctypes.c_float), ("flops", ctypes.c_double),
                ("bytes", ctypes.c_double)]


class Semantics(ctypes.Structure):
    """vy_semantics (include/vyolo.h): the recalled box_nms / BatchNorm choices of one net, each 0 (default) or 1."""
    _fields_ = [("nms_valid_ge", ctypes.c_int32), ("nms_overlap_ge", ctypes.c_int32), ("nms_tie_descending", ctypes.c_int32),
                ("nms_topk_after", ctypes.c_int32), ("nms_iou_plus_one", ctypes.c_int32),
                ("bn_running_var_unbiased", ctypes.c_int32), ("reserved", ctypes.c_int32 * 10)]


class PlanRegion(ctypes.Structure):
    """vy_plan_region (include/vyolo.h): one carve of a workspace plan.  Tests only."""
    _fields_ = [("name", ctypes.c_char * 96), ("offset", ctypes.c_size_t), ("bytes", ctypes.c_size_t), ("span", ctypes.c_size_t)]


VY_PLAN_CLIP, VY_PLAN_TRAIN, VY_PLAN_VIDEO, VY_PLAN_HIER_VIDEO = 0, 1, 2, 3
VY_ERR_RANGE = -5

_vp, _i32, _f32, _sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_size_t

# name -> (restype, argtypes); the single source of truth for the exported-symbols test
SIGNATURES = {
    "vy_last_error": (ctypes.c_char_p, []),
    "vy_version": (ctypes.c_char_p, []),
    "vy_net_create": (ctypes.c_int, [_i32, ctypes.POINTER(_vp)]),
    "vy_net_destroy": (None, [_vp]),
    "vy_net_set_nms": (ctypes.c_int, [_vp, _f32, _i32, _i32]),
    "vy_net_set_semantics": (ctypes.c_int, [_vp, ctypes.POINTER(Semantics)]),
    "vy_net_get_semantics": (ctypes.c_int, [_vp, ctypes.POINTER(Semantics)]),
    "vy_net_num_params": (_i32, [_vp]),
    "vy_net_param_info": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(ParamInfo)]),
    "vy_net_num_convs": (_i32, [_vp]),
    "vy_net_conv_info": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(ConvInfo)]),
    "vy_net_param_bytes": (_sz, [_vp]),
    "vy_net_bind_params": (ctypes.c_int, [_vp, _vp]),
    "vy_net_param_set": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "vy_net_param_get": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "vy_net_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32]),
    "vy_net_bind_workspace": (ctypes.c_int, [_vp, _vp, _sz, _i32, _i32, _i32, _vp]),
    "vy_net_set_keep_activations": (ctypes.c_int, [_vp, _i32]),
    "vy_net_set_conv_mode": (ctypes.c_int, [_vp, _i32]),
    "vy_net_get_conv_mode": (_i32, [_vp]),
    "vy_net_invalidate_split_weights": (ctypes.c_int, [_vp]),
    "vy_net_streamk_state": (ctypes.c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_sz), ctypes.POINTER(_i32)]),
    "vy_net_num_anchors": (_i32, [_vp]),
    "vy_net_forward_infer": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_net_detect_heads": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_net_read_head": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "vy_net_read_activation": (ctypes.c_int, [_vp, ctypes.c_char_p, _vp, ctypes.POINTER(_i32),
                                              ctypes.POINTER(_i32), ctypes.POINTER(_i32), _vp]),
    "vy_net_profile_infer": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.POINTER(LaunchStat),
                                            ctypes.POINTER(_i32), _vp]),
}

ALLREDUCE_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)
GRAD_BUCKET_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64)

SIGNATURES.update({
    "vy_stream_create": (ctypes.c_int, [ctypes.POINTER(_vp)]),
    "vy_stream_destroy": (ctypes.c_int, [_vp]),
    "vy_prefetch_targets": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_preprocess_frames": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vy_preprocess_resize_frames": (ctypes.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vy_net_train_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32]),
    "vy_net_bind_train": (ctypes.c_int, [_vp, _vp, _sz, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vy_net_plan_region": (ctypes.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(PlanRegion)]),
    "vy_net_set_train_options": (ctypes.c_int, [_vp, _f32, _i32]),
    "vy_net_train_forward": (ctypes.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_net_train_mode_forward": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_net_train_backward": (ctypes.c_int, [_vp, _vp, _vp]),
    "vy_net_param_set_opt": (ctypes.c_int, [_vp, _i32, _f32, _f32, _i32]),
    "vy_net_sgd_step": (ctypes.c_int, [_vp, _f32, _f32, _f32, _f32, _vp]),
    "vy_net_grad_get": (ctypes.c_int, [_vp, _i32, _vp, _vp]),
    "vy_net_read_grad_activation": (ctypes.c_int, [_vp, ctypes.c_char_p, _vp, _vp]),
    "vy_net_read_train_tap": (ctypes.c_int, [_vp, ctypes.c_char_p, _i32, _vp, ctypes.POINTER(_i32), _vp]),
    "vy_net_train_conv_plan": (ctypes.c_int, [_vp, _i32, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "vy_net_set_sync_bn": (ctypes.c_int, [_vp, _i32, ALLREDUCE_CB, _vp]),
    "vy_net_set_grad_bucket_cb": (ctypes.c_int, [_vp, GRAD_BUCKET_CB, _vp]),
    # heads-only nets and route tensors (yolo3_no_backbone)
    "vy_net_create_heads": (ctypes.c_int, [_i32, ctypes.POINTER(_vp)]),
    "vy_net_forward_features": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_net_forward_infer_routes": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_net_train_forward_routes": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_net_train_mode_forward_routes": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vy_net_train_backward_routes": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    # k-frame clip nets (yolo3_darknet53 with k > 1, early join)
    "vy_net_create_window": (ctypes.c_int, [_i32, _i32, _i32, ctypes.POINTER(_vp)]),
    "vy_net_window": (ctypes.c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    # hierarchical nets: frames max-pooled by threes inside the backbone (yolo3_darknet53 with new_model / hierarchical)
    "vy_net_create_hier": (ctypes.c_int, [_i32, _i32, ctypes.POINTER(_vp)]),
    "vy_net_create_hier_join": (ctypes.c_int, [_i32, _i32, _i32, ctypes.POINTER(_vp)]),  # ... or joined by a learned conv
    "vy_net_hier": (ctypes.c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "vy_net_tap_frames": (ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.POINTER(_i32)]),
    # windowed heads-only nets: a bank of stored per-frame routes and a (B, k) table (yolo3_no_backbone with k > 1)
    "vy_net_create_heads_window": (ctypes.c_int, [_i32, _i32, _i32, ctypes.POINTER(_vp)]),
    "vy_net_forward_infer_bank": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, ctypes.POINTER(_i32), _vp, _vp, _vp, _vp, _vp]),
    "vy_net_train_forward_bank": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, ctypes.POINTER(_i32), _vp, _i32, _vp, _vp, _vp, _vp,
                                                 _vp, _vp, _vp]),
    "vy_net_train_mode_forward_bank": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, ctypes.POINTER(_i32), _vp, _vp, _vp, _vp, _vp,
                                                      _vp]),
    # video plans of a window net: the backbone once per frame, routes in a ring (videoyolo_amd/video.py)
    "vy_net_video_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32, _i32]),
    "vy_net_bind_video": (ctypes.c_int, [_vp, _vp, _sz, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vy_net_video_push": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(_i32), _vp]),
    "vy_net_video_detect": (ctypes.c_int, [_vp, ctypes.POINTER(_i32), _vp, _vp, _vp, _vp, _vp]),
    "vy_net_video_read_slot": (ctypes.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
    # hier-video plans of a hierarchical net: each level once per frame, the joins dilated (video.hier_detect_video)
    "vy_net_hier_video_frames": (ctypes.c_int, [_vp, _i32, _i32, ctypes.POINTER(_i32)]),
    "vy_net_hier_video_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32]),
    "vy_net_bind_hier_video": (ctypes.c_int, [_vp, _vp, _sz, _i32, _i32, _i32, _i32, _vp]),
    "vy_net_hier_video_detect": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
})


VY_AUG_BRIGHTNESS, VY_AUG_CONTRAST, VY_AUG_SATURATION, VY_AUG_HUE = 1, 2, 3, 4
VY_AUG_MAX_OPS = 4
VY_AUG_CHUNK = 24


class TrainAug(ctypes.Structure):
    """vy_train_aug (include/vyolo.h): one sample's draw of the training transform."""
    _fields_ = [("src_offset", ctypes.c_int64), ("src_h", _i32), ("src_w", _i32), ("paste_x", _i32), ("paste_y", _i32),
                ("canvas_w", _i32), ("canvas_h", _i32), ("crop_x", _i32), ("crop_y", _i32), ("crop_w", _i32),
                ("crop_h", _i32), ("interp", _i32), ("flip", _i32), ("num_ops", _i32), ("op", _i32 * VY_AUG_MAX_OPS),
                ("a", _f32 * VY_AUG_MAX_OPS), ("b", _f32 * VY_AUG_MAX_OPS), ("hue", (_f32 * 3) * 3)]


VY_MIX_CHUNK = 22


class TrainMix(ctypes.Structure):
    """vy_train_mix (include/vyolo.h): one sample's two sources and mix ratios; src2_offset = -1 for no second source."""
    _fields_ = [("src2_offset", ctypes.c_int64), ("h1", _i32), ("w1", _i32), ("h2", _i32), ("w2", _i32), ("l1", _f32),
                ("l2", _f32)]


SIGNATURES.update({
    # the training transform (videoyolo_amd/transforms.py, csrc/augment.hip)
    "vy_train_transform": (ctypes.c_int, [_vp, ctypes.POINTER(TrainAug), _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vy_train_transform_mix": (ctypes.c_int, [_vp, ctypes.POINTER(TrainAug), ctypes.POINTER(TrainMix), _i32, _i32, _vp, _i32,
                                              _i32, _vp, _vp, _vp, _vp]),
    "vy_math_lanczos4": (None, [_f32, ctypes.POINTER(_f32)]),
})

VY_VID_MAX_RANGES = 8
VY_VID_CHUNK = 64
_i64, _f64 = ctypes.c_int64, ctypes.c_double

SIGNATURES.update({
    # the ImageNet-VID metric's matching step (videoyolo_amd/metrics.py, csrc/vid_metric.hip)
    "vy_vid_match": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _f64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                    _vp, _vp, _i64, _vp, _vp, _vp]),
})

VY_VOC_ROWS_MAX = 1024

SIGNATURES.update({
    # the PASCAL-VOC metric's matching step (videoyolo_amd/metrics.py, csrc/voc_metric.hip)
    "vy_voc_match": (ctypes.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp]),
    # the per-frame mean AP from the match's flags (metrics.FrameMApMetric, csrc/voc_metric.hip)
    "vy_voc_frame_ap": (ctypes.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
})

VY_COCO_ROWS_MAX = 1024
VY_COCO_MAX_THRS, VY_COCO_MAX_RANGES = 16, 8
VY_COCO_CHUNK = 128

SIGNATURES.update({
    # the COCO metric's matching step (videoyolo_amd/metrics.py, csrc/coco_metric.hip)
    "vy_coco_match": (ctypes.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp,
                                     _i32, _vp, _i64, _vp, _vp, _vp]),
})

_lib = None


def load():
    """Load libvyolo.so (built by ``python -m videoyolo_amd.build`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build the HIP library first (python -m videoyolo_amd.build). "
            "videoyolo_amd has no CPU fallback." % LIB_PATH)
    # torch ships its own libamdhip64; it must be the one HIP runtime of the process, so it is
    # loaded first and libvyolo.so binds to it (loading /opt/rocm's copy first leaves torch without
    # a device).  torch is the plumbing for device memory / streams anyway.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise VyError(rc, load().vy_last_error().decode())
