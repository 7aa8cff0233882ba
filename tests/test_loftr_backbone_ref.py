"""CPU: pins the float64 backbone reference (oracle/loftr_backbone.py) that tests/test_loftr_backbone_gpu.py holds every
GPU backbone path to: to the ONNX graph (golden pre-transformer tokens of KAT ii) and to the C restatement
(oracle/loftr_oracle.c) on the other KAT pairs, and checks that each reference mutant -- the reference with one error of
a kind the kernels can make -- moves some entry of some frame family of the GPU test past that test's bar, so a kernel
with that bug fails it.

Measured (largest |mutant - reference| over scale, smallest and largest over the frame families that can show it; the bar
is 1e-3): the six strip seams 0.28 .. 1.6 at the layer of the seam, last rows 0.6 .. 2.2, residual 0.6 .. 4.1, shortcut
phase 0.1 .. 2.8, 1 / 256 2e-3 .. 3.7e-2, image index 1.7 .. 25, ignored stride 0.95 .. 21 (nothing on the white frame
with white padding, as it must be), lost split terms 1.2e-3 .. 9.5e-3 (tokens: 2.8e-3 .. 9.5e-3, the tightest).  Every
mutant is detected on every family that can show it."""
import numpy as np
import pytest

from oracle import loftr_backbone as B
from tests import loftr_frames as FR
from tests import loftr_tokens as TK

ONNX_BAR = 1e-4     # a tenth of the GPU tests' bar
BAR = 1e-3          # the GPU tests' bar: 1e-3 of the entry's scale (channel RMS of its pixel or token, at least 1)


def test_frames_are_what_their_names_say():
    fr = FR.frames()
    assert fr.shape == (7, 480, 640) and fr.dtype == np.uint8 and len(FR.NAMES) == 7
    g = fr[FR.NAMES.index("grid")]
    assert set(np.unique(g)) == {0, 255}
    assert g[:, 127:130].all() and not g[100, 126] and not g[100, 130] and g[63:66].all() and not g[62, 100] and not g[66, 100]
    assert g[:2].all() and g[-2:].all() and g[:, :2].all() and g[:, -2:].all() and not g[2, 2] and not g[-3, -3]
    c = fr[FR.NAMES.index("corners")]
    assert int(c.astype(np.int64).sum()) == 4 * 64 * 255 and c[7, 7] and c[7, -8] and c[-8, 7] and c[-8, -8] and not c[8, 8]
    ck = fr[FR.NAMES.index("checker")]
    assert ck[0, 0] == 0 and ck[0, 1] == 255 and ck[1, 0] == 255 and ck[1, 1] == 0
    assert (fr[FR.NAMES.index("white")] == 255).all()
    assert np.array_equal(fr[FR.NAMES.index("kat_ii")], FR.GOLD["img0_ii"])


def test_reference_reproduces_the_onnx_graph():
    """KAT ii img0 / img1 -> the graph's tok0_ii / tok1_ii: measured gap 4.4e-6, held to 1e-4"""
    G = FR.GOLD
    r = B.run(np.stack([G["img0_ii"], G["img1_ii"]]))
    gap = max(np.abs(r["tok"][0] - G["tok0_ii"]).max(), np.abs(r["tok"][1] - G["tok1_ii"]).max())
    print("\nONNX gap %.2e" % gap)
    assert gap <= ONNX_BAR
    for l, s in enumerate(B.LAYER_SHAPES):
        assert r["act"][l].shape == (2,) + s
    assert r["tok"].shape == (2, 1200, 32)


@pytest.mark.parametrize("name", ["i", "iii", "synth"])
def test_reference_reproduces_the_c_restatement(name):
    """measured: i 9.3e-6, iii 8.1e-6, synth 9.3e-6; the match form (A array + B array) against the C restatement's pair"""
    G = FR.GOLD
    r = B.run(G["img0_" + name][None], G["img1_" + name][None])
    ref = TK.kat_tokens(name)
    gap = max(np.abs(r["tok"][0] - ref[0]).max(), np.abs(r["tok"][1] - ref[1]).max())
    print("\n[%s] |ref - C| %.2e" % (name, gap))
    assert gap <= ONNX_BAR


def test_the_two_forms_and_strides_agree():
    """the extract form, the match form and padded frames give the same reference for the same image"""
    fr, ref = FR.frames(), FR.reference()
    m = B.run(fr[[0, 5]], fr[[2, 6]])
    for k, i in enumerate((0, 5, 2, 6)):
        assert np.array_equal(m["tok"][k], ref["tok"][i]) and np.array_equal(m["act"][0][k], ref["act"][0][i])
    p = B.run(FR.padded(fr[[5]], 704, 1, 255), row_stride=704)
    assert np.array_equal(p["tok"][0], ref["tok"][5])


def _furthest(mutant):
    """per layer 1..4 and for the tokens, the largest error over scale of every frame family"""
    fr, ref = FR.frames(), FR.reference()
    names = FR.NAMES
    if mutant == "image_index":            # the match form of the GPU test: 3 A + 3 B, grid and noise among the B frames
        ia, ib = [0, 1, 6], [5, 2, 3]
        base = B.run(fr[ia], fr[ib])
        mut = B.run(fr[ia], fr[ib], mutant=mutant)
        names = [FR.NAMES[i] for i in ia + ib]
    elif mutant == "stride_ignored":       # row_stride 704, the padding white
        base = ref
        mut = B.run(FR.padded(fr, 704, 1, 255), row_stride=704, mutant=mutant)
    else:
        base = ref
        mut = B.run(fr, mutant=mutant, base=ref)
    rows = []
    for l in range(4):
        rows.append(FR.errors(mut["act"][l], base["act"][l], 1)[1].reshape(len(names), -1).max(1))
    rows.append(FR.errors(mut["tok"], base["tok"], 2)[1].reshape(len(names), -1).max(1))
    return names, rows


@pytest.mark.parametrize("mutant", B.MUTANTS)
def test_mutants_are_caught(mutant):
    """Each mutant must move some entry (a layer or the tokens) of some frame family past the bar the GPU test holds every
    entry to.  The whole table is printed; the tokens alone must pass the bar too on some family, since every path is
    compared on them whatever a family's layers do."""
    names, rows = _furthest(mutant)
    print("\n[%s] largest error over scale (bar %g)" % (mutant, BAR))
    print("  %-8s %s" % ("", " ".join("%9s" % n for n in names)))
    for tag, r in zip(("layer1", "layer2", "layer3", "layer4", "tokens"), rows):
        print("  %-8s %s" % (tag, " ".join("%9.2e" % v for v in r)))
    assert max(float(r.max()) for r in rows) > BAR, mutant
    assert float(rows[4].max()) > BAR, mutant
