"""the three registry lines applied to the IMPORTED reference
(slowfast/models/build.py:9,20-75, video_model_builder.py:24,156-165).  oracle/check_integration_a.py
runs them against the reference itself (where its checkout exists) and, with `--record`, keeps the
reference side of that run as data in tests/golden/integration_a.json; the tests here compare the
HIP model, built from the reference's own configs/ssv2.yaml (tests/golden/ssv2.yaml), against it."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _section_a_lines():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## A."):text.index("## B.")]
    return re.search(r"```python\n(.*?)```", sec, re.S).group(1)


def test_section_a_is_what_the_check_executes():
    """The lines the check script runs are the lines the document shows."""
    doc = [l.split("#")[0].strip() for l in _section_a_lines().splitlines()]
    script = open(os.path.join(ROOT, "oracle", "check_integration_a.py")).read()
    for line in doc[1:]:           # (the first line is the reference's own existing import)
        if line:
            assert any(line == s.split("#")[0].strip() for s in script.splitlines()), line


def test_registry_swap_on_the_imported_reference(golden_dir):
    """The model the swapped registry hands the reference's build_model -- svit_amd.model.SViT(cfg) for
    cfg.MODEL.MODEL_NAME -- matches what the reference's own SViT recorded: the 405 names in order,
    shapes, dtypes, the POOL_KV_STRIDE the constructor writes into the cfg, no_weight_decay(), a strict
    state_dict round trip, the reference optimizer's groups; and it refuses to run on the CPU."""
    import torch
    from svit_amd import config, hip
    from svit_amd.model import MODEL_REGISTRY, SViT
    rec = json.load(open(os.path.join(golden_dir, "integration_a.json")))
    assert rec["ref_class"] == "slowfast.models.video_model_builder.SViT"
    assert rec["cfg_class"].startswith("fvcore.common.config") or rec["cfg_class"].endswith("CfgNode")
    assert rec["n_ref"] == len(rec["names"]) == 405 and rec["numel"] == 34373560
    assert rec["optimizer_groups_hip"] == rec["optimizer_groups_ref"]
    # the reference's get_cfg() + configs/ssv2.yaml + the CPU overrides of oracle/ref_shim.reference_cfg()
    cfg = config.get_cfg()
    cfg.merge_from_file(os.path.join(golden_dir, "ssv2.yaml"))
    cfg.NUM_GPUS = rec["num_gpus"]
    cfg.DATA.NUM_FRAMES = rec["num_frames"]
    cfg.DATA.TRAIN_CROP_SIZE = cfg.DATA.TEST_CROP_SIZE = rec["crop"]
    assert cfg.MODEL.MODEL_NAME == "SViT"
    torch.manual_seed(0)
    hip_model = MODEL_REGISTRY.get(cfg.MODEL.MODEL_NAME)(cfg)
    assert type(hip_model) is SViT
    assert type(hip_model).__module__ + "." + type(hip_model).__name__ == "svit_amd.model.SViT"
    hip_sd = hip_model.state_dict()
    assert list(hip_sd.keys()) == rec["names"]
    assert [list(v.shape) for v in hip_sd.values()] == rec["shapes"]
    assert [str(v.dtype) for v in hip_sd.values()] == rec["dtypes"]
    assert int(sum(v.numel() for v in hip_sd.values())) == rec["numel"]
    assert [list(x) for x in cfg.MVIT.POOL_KV_STRIDE] == rec["pool_kv_stride_ref"]
    assert len(rec["pool_kv_stride_ref"]) == 16
    assert sorted(hip_model.no_weight_decay()) == rec["no_weight_decay_ref"]
    # a state_dict of the reference's layout (seeded values) loads strictly and comes back bit for bit
    g = torch.Generator().manual_seed(0)
    ref_sd = {k: torch.randn(s, generator=g).to(getattr(torch, d.split(".")[-1]))
              for k, s, d in zip(rec["names"], rec["shapes"], rec["dtypes"])}
    missing, unexpected = hip_model.load_state_dict(ref_sd, strict=True)
    assert (list(missing), list(unexpected)) == ([], [])
    back = hip_model.state_dict()
    assert all(torch.equal(back[k], ref_sd[k]) for k in ref_sd)
    # the reference's construct_optimizer groups (optimizer.py:35-60): decayed, then zero-decay
    shapes = {n: tuple(p.shape) for n, p in hip_model.named_parameters()}
    n_zero = sum(1 for n, s in shapes.items() if not hip_model.weight_decayed(n, s))
    assert [[len(shapes) - n_zero, cfg.SOLVER.WEIGHT_DECAY], [n_zero, 0.0]] == rec["optimizer_groups_ref"]
    # without a GPU-resident model it must refuse to run, not fall back
    with pytest.raises(hip.SvitHipError):
        hip_model([torch.zeros(1, 3, rec["num_frames"], rec["crop"], rec["crop"])])
