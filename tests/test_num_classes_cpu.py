"""--num-classes on the CPU: the flag picks the dataset's class count and the model's head."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_and_dataset_take_the_class_count():
    from ddp_amd.data import SyntheticCIFAR100
    from ddp_amd.models import build
    assert build("vgg11", 100).fc1.weight.shape == (100, 512)
    assert build("vgg11").fc1.weight.shape == (10, 512)
    ds = SyntheticCIFAR100(True, n=2000)
    images, labels = ds.cpu_arrays()
    assert images.shape == (2000, 32, 32, 3) and ds.classes == 100
    assert int(labels.min()) == 0 and int(labels.max()) == 99


def test_part1_runs_with_100_classes(tmp_path):
    path = str(tmp_path / "m.jsonl")
    r = subprocess.run([sys.executable, os.path.join(REPO, "part1", "main.py"), "--device", "cpu",
                        "--num-classes", "100", "--max-batches", "2", "--train-size", "64",
                        "--test-size", "16", "--global-batch", "8", "--threads", "2",
                        "--metrics", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    recs = [json.loads(l) for l in open(path) if l.strip()]
    assert recs and all(rec["num_classes"] == 100 for rec in recs)
