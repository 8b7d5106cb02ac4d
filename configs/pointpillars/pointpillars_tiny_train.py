# pointpillars_tiny.py with the training settings of the KITTI configurations (loss, assigner thresholds, optimizer, schedule): the
# model tests/test_pp_head_train_gpu.py trains the head of.  Not a model anyone trains.

class_names = ["Cyclist", "Pedestrian"]
point_cloud_range = [0, -2.56, -2.5, 7.68, 2.56, 0.5]     # 48 x 32 pillars of 0.16 m
voxel_size = [0.16, 0.16, 3]

model = dict(
    type="PointPillarsKITTI",
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
    assigner=dict(matched_threshold=0.5, unmatched_threshold=0.35),
    optimizer=dict(type="Adam", weight_decay=0.0001),
    lr=dict(type="exponential_decay_lr", initial_learning_rate=0.0002, decay_rate=0.8, decay_epoch=15, is_stair=True, max_num_epochs=80,
            batch_size=4),
)

test_cfg = dict(
    nms_pre_max_size=200,
    nms_post_max_size=40,
    nms_score_threshold=0.3,
    nms_iou_threshold=0.1,
)

data = dict(pseudo_image_hw=(32, 48), pseudo_image_channels=64, feature_map_hw=(16, 24))
