# CenterPoint on pillars from raw points, test-sized, with the training settings: a PillarDetector on a 64 x 64 grid (0.2 m cells,
# 12.8 m x 12.8 m), two tasks, a 16 x 16 head, at most 32 objects per sample.  For the training chain raw points + ground truth ->
# augmented points -> voxels -> canvas -> head -> targets -> loss (PillarDetector.train_loss); the keys are those of
# centerpoint_pp_nusc_train.py.

tasks = [
    dict(num_class=1, class_names=["car"]),
    dict(num_class=2, class_names=["pedestrian", "traffic_cone"]),
]

voxel_generator = dict(
    range=[-6.4, -6.4, -5.0, 6.4, 6.4, 3.0],
    voxel_size=[0.2, 0.2, 8],
    max_points_in_voxel=20,
    max_voxel_num=4096,
)

model = dict(
    type="PillarDetector",
    reader=dict(type="PillarFeatureNet", num_filters=[64, 64], num_input_features=5, with_distance=False, voxel_size=(0.2, 0.2, 8),
                pc_range=(-6.4, -6.4, -5.0, 6.4, 6.4, 3.0)),
    backbone=dict(type="PointPillarsScatter", ds_factor=1),
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
    voxel_generator=voxel_generator,
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
    augment=dict(global_rot_noise=[-0.3925, 0.3925], global_scale_noise=[0.95, 1.05], global_translate_std=0.2, min_points_in_gt=2),
    max_voxel_num=2048,
    # the reference's nuScenes schedule: Adam with weight decay 0.01 behind a global-norm clip at 35 (optim.CENTERPOINT_OPTIMIZER), the
    # OneCycle rate and beta1 (optim.OneCycle); graphs.PillarDetector.head_trainer() reads `optimizer`
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

data = dict(points_features=5, pseudo_image_hw=(64, 64), pseudo_image_channels=64)
