# CenterPoint on pillars for nuScenes from the LiDAR frames themselves: centerpoint_pp_nusc_points.py restated, with the multi-sweep
# step of the reference's loader (read_sweep per past sweep and the concatenation, det3d_ms/datasets/pipelines/loading.py:56-80,
# 133-159) in front of the voxel generator.  forward_sweeps(pool of frames [N, 4 or 5] f32, lengths, matrices, time lags) ->
# (dets, count): merge (md_cp_sweeps_merge), then forward(points [N, 5] f32, offsets [B + 1] i32); the whole path runs on the device.

# ten sweeps: the key frame and nine past sweeps, each past sweep without the points within min_distance of the ego vehicle
sweeps = dict(nsweeps=10, min_distance=1.0, order="key_first")

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
    sweeps=sweeps,
)

train_cfg = None

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

data = dict(points_features=5, pseudo_image_hw=(512, 512), pseudo_image_channels=64, sweeps=sweeps)
