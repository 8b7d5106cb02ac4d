# Anchor-based PointPillars for the KITTI Car class on 0.16 m pillars, from raw points, with the training settings of the
# reference model's car_xyres16 configuration: this is pointpillars_car_xyres16_points.py plus train_cfg, the `loss` block
# (focal alpha / gamma, smooth-L1 sigma and code weights, the classification and localisation weights), the direction-loss weight
# and the positive / negative class weights, which det_ops.PointPillarsLoss reads (model.loss(points, offsets, example)), and the
# target assigner's settings: det_ops.assign_targets_batch takes the thresholds (they equal the anchor generators').

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

train_cfg = dict(
    loss=dict(
        classification_loss=dict(alpha=0.25, gamma=2.0),
        localization_loss=dict(sigma=3.0, code_weight=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]),
        classification_weight=1.0,
        localization_weight=2.0,
    ),
    direction_loss_weight=0.2,
    pos_class_weight=1.0,
    neg_class_weight=1.0,
    # the training branch of prep_pointcloud (det_ops.PointCloudAugment, model.train_example): the reference configuration's values
    # (groundtruth_localization_noise_std, groundtruth_rotation_uniform_noise, global_rotation_uniform_noise,
    # global_scaling_uniform_noise, global_random_rotation_range_per_object; global_loc_noise_std is fixed by its dataset builder)
    augment=dict(gt_loc_noise_std=[0.25, 0.25, 0.25], gt_rotation_noise=[-0.15707963267, 0.15707963267],
                 global_rotation_noise=[-0.78539816, 0.78539816], global_scaling_noise=[0.95, 1.05], global_loc_noise_std=[0.2, 0.2, 0.2],
                 global_random_rot_range=[0, 0], num_try=100),
    assigner=dict(matched_threshold=0.6, unmatched_threshold=0.45, sample_positive_fraction=-1, sample_size=512,
                  region_similarity_calculator="nearest_iou_similarity"),
    # the optimizer of the reference's train.py (nn.Adam with weight decay, no gradient clip) and its learning-rate schedule
    # (optim.exponential_decay_lr): the reference configuration's values.  model.head_trainer() reads `optimizer`.
    optimizer=dict(type="Adam", weight_decay=0.0001),
    lr=dict(type="exponential_decay_lr", initial_learning_rate=0.0002, decay_rate=0.8, decay_epoch=15, is_stair=True, max_num_epochs=80,
            batch_size=4),
)

test_cfg = dict(
    nms_pre_max_size=900,
    nms_post_max_size=300,
    nms_score_threshold=0.09,
    nms_iou_threshold=0.01,
    post_center_limit_range=[0, -39.68, -5, 69.12, 39.68, 5],
)

data = dict(pseudo_image_hw=(496, 432), pseudo_image_channels=64, feature_map_hw=(248, 216))
