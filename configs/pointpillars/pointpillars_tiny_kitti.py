# pointpillars_tiny_points.py with the KITTI camera-frame ends (see pointpillars_car_xyres16_kitti.py), for the tests: the crop to the
# image frustum in front, the KITTI result rows with a centre range behind.  Not a model anyone trains.

class_names = ["Cyclist", "Pedestrian"]
point_cloud_range = [0, -2.56, -2.5, 7.68, 2.56, 0.5]     # 48 x 32 pillars of 0.16 m
voxel_size = [0.16, 0.16, 3]

model = dict(
    type="PointPillarsKITTIPoints",
    num_point_features=4,
    use_norm=True,
    voxel_feature_extractor=dict(num_filters=[64], with_distance=False),
    middle_feature_extractor=None,
    num_class=2,
    class_names=class_names,
    voxel_generator=dict(point_cloud_range=point_cloud_range, voxel_size=voxel_size, max_number_of_points_per_voxel=8,
                         max_number_of_voxels=256),
    rpn=dict(layer_nums=[1, 2, 1], layer_strides=[2, 2, 2], num_filters=[16, 16, 32], upsample_strides=[1, 2, 4],
             num_upsample_filters=[16, 16, 16], num_input_filters=64),
    anchor_generators=[
        dict(sizes=[0.6, 1.76, 1.73], strides=[0.32, 0.32, 0.0], offsets=[0.16, -2.4, -1.465], rotations=[0, 1.57],
             matched_threshold=0.5, unmatched_threshold=0.35),
        dict(sizes=[0.6, 0.8, 1.73], strides=[0.32, 0.32, 0.0], offsets=[0.16, -2.4, -1.2], rotations=[0, 1.57],
             matched_threshold=0.5, unmatched_threshold=0.35),
    ],
    anchor_area_threshold=1,
    use_direction_classifier=True,
    encode_background_as_zeros=True,
    use_sigmoid_score=True,
    use_bev=False,
)

train_cfg = None

# the threshold lets a few hundred of the 1 536 anchors through on random weights; 40 survivors at the most
test_cfg = dict(
    nms_pre_max_size=200,
    nms_post_max_size=40,
    nms_score_threshold=0.3,
    nms_iou_threshold=0.1,
    # the KITTI ends: the image-frustum crop in front, the centre range and the image-box filter behind
    remove_outside_points=True,
    lidar_input=False,
    # (x from 1.6 m: a box nearer than that has corners beside or behind the camera, whose image box means nothing)
    post_center_limit_range=[1.6, -2.56, -4.5, 7.68, 2.56, 2.5],
)

data = dict(pseudo_image_hw=(32, 48), pseudo_image_channels=64, feature_map_hw=(16, 24))
