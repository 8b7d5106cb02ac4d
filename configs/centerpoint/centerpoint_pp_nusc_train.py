# CenterPoint on pillars for nuScenes from raw points (0.2 m BEV cells, ten sweeps): the voxel generator, the two-layer pillar feature
# net and the scatter of the reference model in front of the neck and the centre-based head of centerpoint_pp_nusc.py.
# forward(points [N, 5] f32, offsets [B + 1] i32) -> (dets, count); the whole path runs on the device.
# This is centerpoint_pp_nusc_points.py plus the training-target assigner of the reference's training configuration (AssignLabel:
# Gaussian overlap 0.1, at most 500 objects per sample, radius at least 2 cells), which det_ops.CenterPointTargets builds on the device,
# and the loss settings of its CenterHead (train_cfg["loss"]), which det_ops.CenterPointLoss reads.

tasks = [
    dict(num_class=1, class_names=["car"]),
    dict(num_class=2, class_names=["truck", "construction_vehicle"]),
    dict(num_class=2, class_names=["bus", "trailer"]),
    dict(num_class=1, class_names=["barrier"]),
    dict(num_class=2, class_names=["motorcycle", "bicycle"]),
    dict(num_class=2, class_names=["pedestrian", "traffic_cone"]),
]

# the evaluation value of max_voxel_num (the reference trains with 30 000 and evaluates with 60 000)
voxel_generator = dict(
    range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0],
    voxel_size=[0.2, 0.2, 8],
    max_points_in_voxel=20,
    max_voxel_num=60000,
)

model = dict(
    type="PillarDetector",
    reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False, voxel_size=(0.2, 0.2, 8),
                pc_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)),
    backbone=dict(type="PointPillarsScatter", ds_factor=1),
    neck=dict(type="RPN", layer_nums=[3, 5, 5], ds_layer_strides=[2, 2, 2], ds_num_filters=[64, 128, 256],
              us_layer_strides=[0.5, 1, 2], us_num_filters=[128, 128, 128], num_input_features=64),
    bbox_head=dict(
        type="CenterHead",
        in_channels=128 * 3,
        tasks=tasks,
        # head name: (output channels, convs in the branch)
        common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)},
        share_conv_channel=64,
        num_hm_conv=2,
        init_bias=-2.19,
    ),
    voxel_generator=voxel_generator,
)

train_cfg = dict(
    assigner=dict(
        target_assigner=dict(tasks=tasks),
        out_size_factor=4,
        gaussian_overlap=0.1,
        max_objs=500,
        min_radius=2,
    ),
    # CenterHead.loss: the loc-loss weight and one weight per anno_box column (reg 2, height, dim 3, vel 2, rot 2), the reference
    # configuration's values; det_ops.CenterPointLoss.from_config reads them
    loss=dict(weight=0.25, code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0]),
    # the Preprocess step's training values of the reference configuration; det_ops.CenterPointAugment.from_config reads them
    augment=dict(global_rot_noise=[-0.3925, 0.3925], global_scale_noise=[0.95, 1.05], global_translate_std=0, min_points_in_gt=-1),
    # the voxel budget the reference trains with (PillarDetector.loss / train_loss)
    max_voxel_num=30000,
    # the reference's nuScenes schedule: Adam with weight decay 0.01 behind a global-norm clip at 35 (optim.CENTERPOINT_OPTIMIZER), the
    # OneCycle rate and beta1 (optim.OneCycle); graphs.PillarDetector.head_trainer() reads `optimizer`
    optimizer=dict(type="Adam", weight_decay=0.01, max_norm=35.0),
    lr_config=dict(type="OneCycle", lr_max=1e-3, moms=[0.95, 0.85], div_factor=10.0, pct_start=0.4),
)

voxel_size = [0.2, 0.2]
test_cfg = dict(
    post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
    max_per_img=500,
    nms=dict(nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=0.2),
    score_threshold=0.1,
    pc_range=[-51.2, -51.2],
    out_size_factor=4,     # the neck's output stride on the 512 x 512 grid
    voxel_size=voxel_size,
)

data = dict(points_features=5, pseudo_image_hw=(512, 512), pseudo_image_channels=64)
