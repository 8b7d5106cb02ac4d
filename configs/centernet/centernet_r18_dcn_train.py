# centernet_r18_dcn.py plus the training values of the reference's default_config.yaml: the target step of COCOHP.preprocess_fn
# (at most 128 objects per image on the 128 x 128 map, Gaussian min_overlap 0.7), which det_ops.CenterNetTargets builds on the device,
# and the loss settings of CenterNetLossCell (FocalLoss on the heat map, l1 RegLoss on wh and on the offset), which
# det_ops.CenterNetLoss reads, and the augmentation block of its dataset_config (default_config.yaml:61-91: random crop, flip, colour
# augmentation with the PCA lighting terms, the BGR mean and std), which det_ops.CenterNetAugment builds on the device.

model = dict(
    type="CenterNet",
    depth=18,
    num_classes=80,
    head_conv=64,
    K=100,
    dcn=True,
)

train_cfg = dict(
    assigner=dict(input_res=(512, 512), down_ratio=4, max_objs=128, min_overlap=0.7),
    loss=dict(hm_weight=1.0, wh_weight=0.1, off_weight=1.0, reg_offset=True, reg_loss="l1", mse_loss=False, dense_wh=False,
              cat_spec_wh=False, num_stacks=1),
    augment=dict(rand_crop=True, scale=0.4, shift=0.1, flip_prop=0.5, color_aug=True, aug_rot=0.0, rotate=0,
                 eig_val=[0.2141788, 0.01817699, 0.00341571],
                 eig_vec=[[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                          [-0.56089297, 0.71832671, 0.41158938]],
                 mean=[0.40789654, 0.44719302, 0.47026115], std=[0.28863828, 0.27408164, 0.27809835]),
    # default_config.yaml:112-132 (train_config: Adam, the MultiDecay schedule); graphs.CenterNet.head_trainer reads `optimizer`,
    # optim.multi_epochs_decay_lr takes the values of `lr_config`.  The reference's loss_scale_value 1024 is not applied: fp32 gradients.
    optimizer=dict(type="Adam", eps=1e-7, weight_decay=0.0),
    lr_config=dict(type="MultiEpochsDecayLR", learning_rate=5e-4, multi_epochs=[90, 120], factor=10, warmup_steps=0, batch_size=16),
)
test_cfg = dict(K=100, reg_offset=True)

data = dict(input_hw=(512, 512), down_ratio=4)
