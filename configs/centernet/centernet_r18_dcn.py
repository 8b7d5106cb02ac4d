# CenterNet (objects as points) on ResNet-18 with three deformable-conv + deconv stages for COCO, the values of the reference's
# default_config.yaml: 80 classes, 512 x 512 input, output stride 4 (a 128 x 128 map), the 100 best peaks.
# forward(images [B, 512, 512, 8] bf16) -> dets [B, 100, 6]

model = dict(
    type="CenterNet",
    depth=18,
    num_classes=80,
    head_conv=64,
    K=100,
    dcn=True,
)

train_cfg = None
test_cfg = dict(K=100, reg_offset=True)

data = dict(input_hw=(512, 512), down_ratio=4)
