# KITTI PointPillars (Car, 0.16 m pillars) from a raw velodyne scan to KITTI result rows: pointpillars_car_xyres16_points.py with the
# camera-frame ends of the reference's pipeline on the device.  forward_kitti() takes the whole scan and a det_ops.KittiCalibration, cuts
# the scan to the image frustum (remove_outside_points, car_xyres16.yaml), runs the model and writes the rows of predict_kitti_to_anno
# with post_center_limit_range (car_xyres16.yaml:104); prepare_kitti() does the same cut and turns camera-frame labels for training.

class_names = ["Car"]
point_cloud_range = [0, -39.68, -3, 69.12, 39.68, 1]
voxel_size = [0.16, 0.16, 4]

model = dict(
    type="PointPillarsKITTIPoints",
    num_point_features=4,
    use_norm=True,
    voxel_feature_extractor=dict(num_filters=[64], with_distance=False),
    middle_feature_extractor=None,
    num_class=1,
    class_names=class_names,
    voxel_generator=dict(point_cloud_range=point_cloud_range, voxel_size=voxel_size, max_number_of_points_per_voxel=32,
                         max_number_of_voxels=40000),
    # three blocks at strides 2, 4, 8 of the 496 x 432 canvas, every one upsampled back to 248 x 216 and concatenated (384 channels)
    rpn=dict(layer_nums=[3, 5, 5], layer_strides=[2, 2, 2], num_filters=[64, 128, 256], upsample_strides=[1, 2, 4],
             num_upsample_filters=[128, 128, 128], num_input_filters=64),
    # one generator, two rotations -> 2 anchors per cell, 107 136 in all; sizes are (w, l, h), the z entry of strides is not used
    anchor_generators=[
        dict(sizes=[1.6, 3.9, 1.56], strides=[0.32, 0.32, 0.0], offsets=[0.16, -39.52, -1.78], rotations=[0, 1.57],
             matched_threshold=0.6, unmatched_threshold=0.45),
    ],
    anchor_area_threshold=1,
    use_direction_classifier=True,
    encode_background_as_zeros=True,
    use_sigmoid_score=True,
    use_bev=False,
)

train_cfg = None

test_cfg = dict(
    nms_pre_max_size=900,
    nms_post_max_size=300,
    nms_score_threshold=0.09,
    nms_iou_threshold=0.01,
    # the KITTI ends: remove_outside_points and lidar_input of car_xyres16.yaml's readers, post_center_limit_range of :104
    remove_outside_points=True,
    lidar_input=False,
    post_center_limit_range=[0, -39.68, -5, 69.12, 39.68, 5],
)

data = dict(pseudo_image_hw=(496, 432), pseudo_image_channels=64, feature_map_hw=(248, 216))
