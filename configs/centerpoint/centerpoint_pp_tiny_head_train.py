# CenterPoint on pillars at the pseudo-image level, test-sized, with the training settings: the neck and the head of
# centerpoint_pp_tiny_points_train.py behind a 64 x 64 pseudo-image (0.2 m cells, 12.8 m x 12.8 m), two tasks (12 SepHead branches), a
# 16 x 16 head, at most 32 objects per sample.  For the head's training step (graphs.PointPillars.train_step: pseudo-image + targets ->
# updated head); the keys are those of centerpoint_pp_nusc_train.py.

tasks = [
    dict(num_class=1, class_names=["car"]),
    dict(num_class=2, class_names=["pedestrian", "traffic_cone"]),
]

# the grid the pseudo-image stands for (det_ops.CenterPointTargets reads the range and the voxel size; the model takes the canvas itself)
voxel_generator = dict(
    range=[-6.4, -6.4, -5.0, 6.4, 6.4, 3.0],
    voxel_size=[0.2, 0.2, 8],
    max_points_in_voxel=20,
    max_voxel_num=4096,
)

model = dict(
    type="PointPillars",
    neck=dict(type="RPN", layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256],
              us_layer_strides=[0.5, 1, 2], us_num_filters=[128, 128, 128], num_input_features=64),
    bbox_head=dict(
        type="CenterHead",
        in_channels=128 * 3,
        tasks=tasks,
        common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)},
        share_conv_channel=64,
        num_hm_conv=2,
        init_bias=-2.19,
    ),
)

train_cfg = dict(
    assigner=dict(
        target_assigner=dict(tasks=tasks),
        out_size_factor=4,
        gaussian_overlap=0.1,
        max_objs=32,
        min_radius=2,
    ),
    loss=dict(weight=0.25, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0]),
    optimizer=dict(type="Adam", weight_decay=0.01, max_norm=35.0),
    lr_config=dict(type="OneCycle", lr_max=1e-3, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4),
)

voxel_size = [0.2, 0.2]
test_cfg = dict(
    post_center_limit_range=[-8.0, -8.0, -10.0, 8.0, 8.0, 10.0],
    max_per_img=100,
    nms=dict(nms_pre_max_size=128, nms_post_max_size=20, nms_iou_threshold=0.2),
    score_threshold=0.1,
    pc_range=[-6.4, -6.4],
    out_size_factor=4,
    voxel_size=voxel_size,
)

data = dict(pseudo_image_hw=(64, 64), pseudo_image_channels=64)
