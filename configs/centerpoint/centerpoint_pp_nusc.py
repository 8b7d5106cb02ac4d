# CenterPoint on pillars for nuScenes (0.2 m BEV cells, ten sweeps): the RPN neck and the centre-based head of the reference model,
# with the post-processing settings of its test configuration.  The pillar encoder and the scatter that make the 512 x 512 x 64
# pseudo-image are not part of this build, so the model has no `reader` / `backbone` entry: forward() takes the pseudo-image.

# six detection tasks; each owns a heat-map channel per class
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
        # head name: (output channels, convs in the branch)
        common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)},
        share_conv_channel=64,
        num_hm_conv=2,
        init_bias=-2.19,
    ),
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

data = dict(pseudo_image_hw=(512, 512), pseudo_image_channels=64)
