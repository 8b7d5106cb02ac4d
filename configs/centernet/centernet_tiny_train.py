# A small CenterNet for tests of the training chain (graphs.CenterNet.train_example / train_loss): ResNet-18 without the deformable
# layers, 5 classes, a 64 x 96 input (a 16 x 24 map at down_ratio 4: not the one-launch stem's extent, so the input is [B,64,96,8]),
# at most 8 objects per image.  The augmentation and loss values are those of centernet_r18_dcn_train.py.

model = dict(
    type="CenterNet",
    depth=18,
    num_classes=5,
    head_conv=64,
    K=20,
    dcn=False,
)

train_cfg = dict(
    assigner=dict(input_res=(64, 96), down_ratio=4, max_objs=8, min_overlap=0.7),
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
test_cfg = dict(K=20, reg_offset=True)

data = dict(input_hw=(64, 96), down_ratio=4)
