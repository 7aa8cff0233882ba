"""Float64 restatement of the LoFTR ResNet backbone (ConvertImageToFloat, 21 convolutions, positional encoding) -- TEST
INFRASTRUCTURE ONLY.  The graph as in oracle/loftr_oracle.c (loftr_oracle_run): input u8 * f32(1 / 255); conv00 (7 x 7,
stride 2, pad 3); four layers of two BasicBlocks, out = relu(conv_b(relu(conv_a(x))) + residual), the first block of
layers 2..4 with a stride-2 conv_a and a 1 x 1 stride-2 shortcut as residual (conv07, conv12, conv17); outconv without
bias; + pe; n c h w -> n (h w) c.  torch.nn.functional.conv2d in float64 on the CPU.  Pinned by
tests/test_loftr_backbone_ref.py to tests/golden/loftr_kat.npz and to the C restatement;
tests/test_loftr_backbone_gpu.py holds every GPU backbone path to it.

run(frames_a, frames_b=None, row_stride=640, mutant=None) takes the frames as a backbone pass does: two arrays of
u8 frames [n][480][row_stride] (the second may be absent), and returns {"act": [layer1..layer4 as (n, C, H, W)],
"tok": (n, 1200, 32)} over the A frames followed by the B frames, in float64.

A mutant is the reference with one deliberate error of a kind the kernels can make (MUTANTS):

* seam_<kernel>: the intermediate t of the BasicBlock that streaming kernel computes is read as zero at the first
  column of its second strip: column 64 at 320 wide (k_stem_strip8x, k_strip8x), 32 at 160 wide (k_down16x, k_strip16x),
  16 at 80 wide (k_down32x, k_strip32x).
* last_rows_down32x: the last row pair of t is missing in k_down32x's block (layer 3, block 1).
* residual_l1b2: block 2 of layer 1 takes its residual from the stem's output instead of block 1's.
* shortcut_phase: the conv07 shortcut samples odd columns.
* scale_256: the input scale is 1 / 256.
* image_index: image k of the B array computes frame k - 1 of it (image 0 the last).
* stride_ignored: row_stride is ignored, the rows of a frame are read 640 bytes apart.
* split_drop_hi_lo: conv13 as a split-bf16 product that keeps hi . hi and lo . hi but has lost hi . lo (activation hi
  times weight lo), the operands rounded with torch.bfloat16.
"""
import os
import struct

import numpy as np

H, W = 480, 640
NTOK, DM = 1200, 32
WEIGHTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mono_slam_framework_amd", "weights",
                       "loftr_teacher.bin")
LAYER_SHAPES = [(8, 240, 320), (16, 120, 160), (32, 60, 80), (32, 30, 40)]
SEAMS = {"seam_stem_strip8x": (1, 64), "seam_strip8x": (3, 64), "seam_down16x": (5, 32), "seam_strip16x": (8, 32),
         "seam_down32x": (10, 16), "seam_strip32x": (13, 16)}      # mutant -> (conv_a of the block, column of t)
MUTANTS = tuple(SEAMS) + ("last_rows_down32x", "residual_l1b2", "shortcut_phase", "scale_256", "image_index",
                          "stride_ignored", "split_drop_hi_lo")
# the first layer (1..4; 0 = the input) a mutant changes: run(base=) reuses the clean layers before it
FIRST_LAYER = {"seam_stem_strip8x": 1, "seam_strip8x": 1, "seam_down16x": 2, "seam_strip16x": 2, "seam_down32x": 3,
               "seam_strip32x": 3, "last_rows_down32x": 3, "residual_l1b2": 1, "shortcut_phase": 2, "scale_256": 0,
               "image_index": 0, "stride_ignored": 0, "split_drop_hi_lo": 3}

_W = None


def weights(path=WEIGHTS):
    """{"conv%02d.w", "conv%02d.b" (where the blob has one), "outconv.w", "pe"} as float64 torch tensors"""
    global _W
    if _W is not None and path == WEIGHTS:
        return _W
    import torch
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != b"MSFLTR01":
        raise IOError("not an MSFLTR01 blob: " + path)
    n = struct.unpack_from("<I", raw, 8)[0]
    recs, o = {}, 12
    for _ in range(n):
        name, nd, d0, d1, d2, d3, off, cnt = struct.unpack_from("<32sI4III", raw, o)
        o += 60
        recs[name.rstrip(b"\0").decode()] = ((d0, d1, d2, d3)[:nd], off, cnt)
    data = np.frombuffer(raw, np.float32, offset=o)
    out = {}
    for k, (shape, off, cnt) in recs.items():
        if k.startswith("conv") or k.startswith("outconv") or k == "pe":
            out[k] = torch.from_numpy(data[off:off + cnt].reshape(shape).astype(np.float64))
    if path == WEIGHTS:
        _W = out
    return out


def _images(frames, row_stride, mutant):
    """u8 [n][480][row_stride] -> [n][480][640] as the (mutant) kernel addresses them"""
    f = np.ascontiguousarray(frames, np.uint8)
    n = f.shape[0]
    f = f.reshape(n, -1)
    assert f.shape[1] >= H * row_stride and row_stride >= W
    if mutant == "stride_ignored":
        return f[:, :H * W].reshape(n, H, W)
    return f[:, :H * row_stride].reshape(n, H, row_stride)[:, :, :W]


def run(frames_a, frames_b=None, row_stride=W, mutant=None, base=None):
    """base: the result of a clean run on the same frames; layers the mutant cannot change are taken from it"""
    import torch
    import torch.nn.functional as F
    assert mutant is None or mutant in MUTANTS, mutant
    Wt = weights()
    first = FIRST_LAYER[mutant] if mutant else 0

    def conv(i, x, stride=1, relu=True, res=None, w=None):
        name = "conv%02d" % i if i < 20 else "outconv"
        w = Wt[name + ".w"] if w is None else w
        y = F.conv2d(x, w, Wt.get(name + ".b"), stride=stride, padding=w.shape[-1] // 2)
        if res is not None:
            y = y + res
        return torch.relu(y) if relu else y

    def seam(i, t):
        if mutant in SEAMS and SEAMS[mutant][0] == i:
            t = t.clone()
            t[..., SEAMS[mutant][1]] = 0
        return t

    def block(ia, ib, x, res):
        t = seam(ia, conv(ia, x))
        return conv(ib, t, res=res)

    def down(ia, ib, isc, x):
        xs = x[..., 1:] if (mutant == "shortcut_phase" and isc == 7) else x
        sc = conv(isc, xs, stride=2, relu=False)
        t = seam(ia, conv(ia, x, stride=2))
        if mutant == "last_rows_down32x" and ia == 10:
            t = t.clone()
            t[..., -2:, :] = 0
        return conv(ib, t, res=sc)

    act = [None] * 4
    with torch.no_grad():
        if base is not None and first >= 2:
            for l in range(first - 1):
                act[l] = torch.from_numpy(np.array(base["act"][l]))
        else:
            imgs = [_images(frames_a, row_stride, mutant)]
            if frames_b is not None:
                b = _images(frames_b, row_stride, mutant)
                imgs.append(np.roll(b, 1, axis=0) if mutant == "image_index" else b)
            u8 = np.concatenate(imgs, 0)
            k = np.float32(1.0 / 256.0) if mutant == "scale_256" else np.float32(1.0 / 255.0)
            x = torch.from_numpy(u8.astype(np.float64) * np.float64(k))[:, None]      # u8 * f32(1 / 255), exact in f64
            s = conv(0, x, stride=2)
            b1 = block(1, 2, s, s)
            act[0] = block(3, 4, b1, s if mutant == "residual_l1b2" else b1)
        if act[1] is None:
            d = down(5, 6, 7, act[0])
            act[1] = block(8, 9, d, d)
        if act[2] is None:
            d = down(10, 11, 12, act[1])
            t = seam(13, conv(13, d))
            if mutant == "split_drop_hi_lo":
                w = Wt["conv13.w"]
                wh = w.float().bfloat16().double()
                dh = d.float().bfloat16().double()
                dl = (d.float() - dh.float()).bfloat16().double()
                t = seam(13, conv(13, dh + dl, w=wh))
            act[2] = conv(14, t, res=d)
        d = down(15, 16, 17, act[2])
        act[3] = block(18, 19, d, d)
        o = conv(20, act[3], relu=False) + Wt["pe"].reshape(1, DM, 30, 40)
        tok = o.reshape(o.shape[0], DM, NTOK).permute(0, 2, 1).contiguous()
    return {"act": [a.numpy() for a in act], "tok": tok.numpy()}


def scale_of(ref, axis):
    """the scale an entry's error is measured against: the RMS over the channels of its pixel or token, at least 1"""
    return np.maximum(1.0, np.sqrt((np.asarray(ref, np.float64) ** 2).mean(axis, keepdims=True)))
