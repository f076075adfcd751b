"""Pin the numpy oracle against the committed reference outputs (CPU only)."""
import numpy as np
import pytest

from oracle import uvl_oracle as O
from tests.golden_util import list_cases, load_case, rebuild_inputs, rebuild_weights

ATOL = 2e-4     # fp32 re-association only; measured deviation is <= 1.5e-5 (see fixture meta)

SMALL = [c for c in list_cases() if c.startswith("tiny")]
BIG = [c for c in list_cases() if not c.startswith("tiny")]


def _check(name):
    meta, spec, ref = load_case(name)
    inp = rebuild_inputs(meta, spec)
    sd = rebuild_weights(meta, spec)
    out = O.forward_test(sd, spec, inp["template"], inp["search"], inp["ids"], inp["mask"], inp["prompt"], inp["flag"])
    for k, v in ref.items():
        if k == "flag":
            assert (out["flag"] == v).all()
            continue
        if k == "prompt_init" or k.startswith("fwd."):     # covered by the prompter / UVLTrack.forward tests below
            continue
        if k.endswith(".slice"):
            got = out[k[:-6]][:, :8, :32]
        else:
            got = out[k]
        assert got.shape == v.shape, k
        np.testing.assert_allclose(got, v, atol=ATOL, rtol=0, err_msg="%s/%s" % (name, k))


@pytest.mark.parametrize("name", SMALL)
def test_oracle_matches_reference_tiny(name):
    _check(name)


def _check_torch(name):
    """oracle/uvl_oracle_torch.py (the ATen-operator form bench.py's cpu_baseline times) against the same reference outputs, same gate"""
    from oracle import uvl_oracle_torch as OT
    meta, spec, ref = load_case(name)
    inp = rebuild_inputs(meta, spec)
    sd = rebuild_weights(meta, spec)
    out = OT.forward_test(sd, spec, inp["template"], inp["search"], inp["ids"], inp["mask"], inp["prompt"], inp["flag"])
    n = 0
    for k, v in ref.items():
        if k == "flag" or k == "prompt_init" or k.startswith("fwd."):
            continue
        got = out[k[:-6]][:, :8, :32] if k.endswith(".slice") else out[k]
        assert got.shape == v.shape, k
        np.testing.assert_allclose(got, v, atol=ATOL, rtol=0, err_msg="torch oracle %s/%s" % (name, k))
        n += 1
    assert n >= 8


@pytest.mark.parametrize("name", SMALL)
def test_torch_oracle_matches_reference_tiny(name):
    _check_torch(name)


@pytest.mark.slow
@pytest.mark.parametrize("name", ["b_z128_x256", "b_z256_x256"])
def test_torch_oracle_matches_reference_base(name):
    _check_torch(name)


@pytest.mark.slow
@pytest.mark.parametrize("name", [c for c in BIG if c.startswith("b_") and not c.endswith("_b32")])      # (the 32-sequence fixture is the same code on 32 samples: minutes
def test_oracle_matches_reference_base(name):                                                             #  of numpy; its deviation, 4.2e-5, is recorded in its meta at generation)
    _check(name)


@pytest.mark.parametrize("name", SMALL)
def test_oracle_prompter_matches_reference(name):
    """forward_prompt_init (backbone + DistributionBasedCrossAttention) against the reference's own output."""
    meta, spec, ref = load_case(name)
    inp = rebuild_inputs(meta, spec)
    sd = rebuild_weights(meta, spec, include_unused=True)
    tem_mask, ctx_mask = O.box_masks(spec, meta["batch"], seed=meta["input_seed"])
    got = O.forward_prompt_init(sd, spec, inp["template"], inp["search"], inp["ids"], inp["mask"], tem_mask, ctx_mask, inp["flag"])
    assert got.shape == ref["prompt_init"].shape == (meta["batch"], 3, spec.dim)
    np.testing.assert_allclose(got, ref["prompt_init"], atol=ATOL, rtol=0)
    # flag 1 (grounding) returns the un-updated queries: query_embed (+ token on row 0), independent of the masks
    for b, fl in enumerate(meta["flags"]):
        if fl == 1:
            other = O.forward_prompt_init(sd, spec, inp["template"], inp["search"], inp["ids"], inp["mask"], ~tem_mask, ~ctx_mask, inp["flag"])
            np.testing.assert_array_equal(other[b], got[b])


@pytest.mark.parametrize("name", SMALL)
def test_oracle_forward_matches_reference(name):
    """UVLTrack.forward in eval mode (the grounding call; head on its no-prompt branch, cont_score with two channels)."""
    meta, spec, ref = load_case(name)
    inp = rebuild_inputs(meta, spec)
    sd = rebuild_weights(meta, spec, include_unused=True)
    tem_mask, ctx_mask = O.box_masks(spec, meta["batch"], seed=meta["input_seed"])
    out = O.forward(sd, spec, inp["template"], inp["search"], inp["ids"], inp["mask"], tem_mask, ctx_mask, inp["flag"])
    assert out["cont_score"].shape == (meta["batch"], spec.nx, 2)
    for k in ("cont_score", "bbox_map", "pred_boxes", "cls_score", "cls_score_test", "prompts"):
        np.testing.assert_allclose(out[k], ref["fwd." + k], atol=ATOL, rtol=0, err_msg="%s/fwd.%s" % (name, k))


def _decode_fixture():
    """The reference's own clip_box and UVLTrack.track post-processing, run on seeded random inputs by oracle/make_decode_golden.py:
    inputs and outputs stored in tests/golden/tracker/decode_reference.npz."""
    import os
    from tests.golden_util import GOLDEN_DIR
    return np.load(os.path.join(GOLDEN_DIR, "tracker", "decode_reference.npz"))


def test_oracle_clip_box_matches_reference_when_available():
    """tracker decode row: clip_box is pinned against the stored outputs of the reference's own function (lib/utils/box_ops.py:117-126)."""
    z = _decode_fixture()
    boxes, hw, want = z["clip.box"], z["clip.hw"], z["clip.out"]
    assert len(boxes) == len(hw) == len(want) == 200
    for box, (H, W), ref in zip(boxes, hw, want):
        assert O.clip_box(box.tolist(), int(H), int(W), margin=10) == ref.tolist()


def test_tracker_decode_against_reference_lines():
    """The rest of the decode row: the reference's own post-processing statements of UVLTrack.track
    (lib/test/tracker/uvltrack.py:116-125) and its map_box_back (:167-173), executed by oracle/make_decode_golden.py on random head
    outputs (nothing is copied into this repository); oracle.tracker_decode must reproduce the stored box, score and argmax."""
    z = _decode_fixture()
    for F in (16, 24):
        p = "decode.f%d." % F
        search_size = int(z[p + "search_size"])
        window = O.hann_window(F)
        assert len(z[p + "cls"]) == 20
        for t in range(len(z[p + "cls"])):
            cls, cont, bbox = z[p + "cls"][t:t + 1], z[p + "cont"][t:t + 1], z[p + "bbox"][t:t + 1]
            assert cls.shape == (1, F, F) and cont.shape == (1, F * F, 3) and bbox.shape == (1, F * F, 4)
            state, rf, (H, W) = z[p + "state"][t], float(z[p + "rf"][t]), z[p + "hw"][t]
            e_state, e_score, e_net, e_idx = O.tracker_decode(cls, cont, bbox, window, np.asarray([state], np.float32), np.asarray([rf], np.float32),
                                                              np.asarray([[H, W]], np.float32), search_size)
            np.testing.assert_allclose(z[p + "out_state"][t], e_state[0], rtol=0, atol=2e-4)
            assert abs(float(z[p + "out_score"][t]) - float(e_score[0])) < 1e-6
            np.testing.assert_array_equal(z[p + "out_net"][t], e_net[0])


def test_hann_window_shape_and_symmetry():
    w = O.hann_window(16).reshape(16, 16)
    assert w.shape == (16, 16) and np.allclose(w, w.T) and w[0].max() == 0.0 and abs(w.max() - np.hanning(16).max() ** 2) < 1e-7


def test_mask_semantics_text_never_leaks_in_bbox_mode():
    """flag 0 masks every text key (extractor.py:43-50): visual outputs must not depend on the text ids."""
    meta, spec, _ = load_case("tiny_mixed")
    inp = rebuild_inputs(meta, spec)
    sd = rebuild_weights(meta, spec)
    flag = np.zeros_like(inp["flag"])
    a = O.forward_test(sd, spec, inp["template"], inp["search"], inp["ids"], inp["mask"], inp["prompt"], flag)
    ids2 = (inp["ids"] + 7) % spec.vocab
    b = O.forward_test(sd, spec, inp["template"], inp["search"], ids2, inp["mask"], inp["prompt"], flag)
    for k in ("search", "bbox_map", "cls_score_test", "cont_score", "logits"):
        np.testing.assert_array_equal(a[k], b[k])
    assert np.abs(a["text"] - b["text"]).max() > 1e-3


def test_batch_independence():
    """Each sequence is independent in eval mode: batch of 3 == 3 single runs."""
    meta, spec, _ = load_case("tiny_mixed")
    inp = rebuild_inputs(meta, spec)
    sd = rebuild_weights(meta, spec)
    full = O.forward_test(sd, spec, inp["template"], inp["search"], inp["ids"], inp["mask"], inp["prompt"], inp["flag"])
    for b in range(meta["batch"]):
        one = O.forward_test(sd, spec, inp["template"][b:b + 1], inp["search"][b:b + 1], inp["ids"][b:b + 1],
                             inp["mask"][b:b + 1], inp["prompt"][b:b + 1], inp["flag"][b:b + 1])
        for k in ("bbox_map", "cls_score_test", "cont_score", "logits", "search"):
            np.testing.assert_allclose(one[k][0], full[k][b], atol=1e-5, rtol=0)
