# centernet_r18_dcn.py plus the training values of the reference's default_config.yaml: the target step of COCOHP.preprocess_fn
# (at most 128 objects per image on the 128 x 128 map, Gaussian min_overlap 0.7), which det_ops.CenterNetTargets builds on the device,
# and the loss settings of CenterNetLossCell (FocalLoss on the heat map, l1 RegLoss on wh and on the offset), which
# det_ops.CenterNetLoss reads.

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
)
test_cfg = dict(K=100, reg_offset=True)

data = dict(input_hw=(512, 512), down_ratio=4)
