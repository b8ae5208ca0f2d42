"""GPU: scripts/compute_branches.py on a directory of Z stacks with --detect-well and --tree-visualizations: the batch path (one upload
per chunk, masks from the resident chunk, geometry and overlays out of the batch call) and TMAT_STACK_BATCH=0 (every stack on the
per-stack path) write the same CSV bytes, the same file names and the same pictures, and the batch path is really taken."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import well_stacks as ws  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
SCRIPT = REPO / "tissue-model-analysis-tools_amd" / "scripts" / "compute_branches.py"


def run(args, env_extra=None):
    env = dict(os.environ, TMAT_SYNTHETIC_WEIGHTS="1")
    env.pop("TMAT_STACK_BATCH", None)
    env.pop("TMAT_TRACE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, str(SCRIPT)] + args, capture_output=True, text=True, env=env, timeout=600)


def test_both_flags_through_the_batch_path_write_the_per_stack_files(tmp_path):
    """the directory of test_gpu_stack_batch_script.py -- s0, s1 and s3 share a shape, s2 (between them) has another: chunks [s0, s1],
    [s2], [s3] -- with wells on s0 (a fitted mask that prunes) and s1 (rejected by the coverage rule)"""
    from PIL import Image
    from tmat_amd import synth
    ind = tmp_path / "in"
    ind.mkdir()
    stacks = {"s0": ws.well_stack(40), "s1": ws.well_stack(41), "s2": synth.synth_stack(82, 4, 150, 140, n_vessels=6),
              "s3": synth.synth_stack(83, 3, 128, 160, n_vessels=6)}
    for k, st in stacks.items():
        for z, sl in enumerate(st):
            Image.fromarray(sl).save(ind / f"{k}_z{z}.tif")
    flags = ["--image-width-microns", "800", "--graph-thresh-1", "2", "5", "-w", "--tree-visualizations", "--visualizations", "--vis-width", "200"]
    outs, res = {}, {}
    for name, env in (("default", {"TMAT_TRACE": "1"}), ("single", {"TMAT_STACK_BATCH": "0"})):
        outs[name] = tmp_path / name
        res[name] = run([str(ind), str(outs[name])] + flags, env)
        assert res[name].returncode == 0, res[name].stdout + res[name].stderr
    assert any("stack pass" in ln and "(2 stacks)" in ln for ln in res["default"].stderr.splitlines()), res["default"].stderr
    want = sorted(p.relative_to(outs["single"]) for p in outs["single"].rglob("*") if p.is_file())
    pngs = [p for p in want if p.suffix == ".png"]
    assert len([p for p in want if p.suffix == ".csv"]) == 2
    assert sum(p.name == "well_mask.png" for p in pngs) == 4 and sum(p.name.startswith("morse_tree") for p in pngs) >= 6
    assert sorted(p.relative_to(outs["default"]) for p in outs["default"].rglob("*") if p.is_file()) == want
    for rel in want:
        a, b = outs["default"] / rel, outs["single"] / rel
        if rel.suffix == ".csv":
            assert a.read_bytes() == b.read_bytes(), rel
            assert len(a.read_bytes().decode("utf-16").strip().splitlines()) == 5
        elif rel.suffix == ".png":
            assert np.array_equal(np.array(Image.open(a)), np.array(Image.open(b))), rel
