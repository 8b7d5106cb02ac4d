# CenterPoint on pillars, test-sized: the six tasks, the neck and the head of centerpoint_pp_nusc.py on a 128 x 128 pseudo-image
# (0.2 m cells, 25.6 m x 25.6 m), so the head sees 32 x 32 = 1 024 BEV cells; 256 candidates per task before the NMS, 20 after.

tasks = [
    dict(num_class=1, class_names=["car"]),
    dict(num_class=2, class_names=["truck", "construction_vehicle"]),
    dict(num_class=2, class_names=["bus", "trailer"]),
    dict(num_class=1, class_names=["barrier"]),
    dict(num_class=2, class_names=["motorcycle", "bicycle"]),
    dict(num_class=2, class_names=["pedestrian", "traffic_cone"]),
]

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

train_cfg = None

voxel_size = [0.2, 0.2]
test_cfg = dict(
    post_center_limit_range=[-15.0, -15.0, -10.0, 15.0, 15.0, 10.0],
    max_per_img=500,
    nms=dict(nms_pre_max_size=256, nms_post_max_size=20, nms_iou_threshold=0.2),
    score_threshold=0.1,
    pc_range=[-12.8, -12.8],
    out_size_factor=4,
    voxel_size=voxel_size,
)

data = dict(pseudo_image_hw=(128, 128), pseudo_image_channels=64)
