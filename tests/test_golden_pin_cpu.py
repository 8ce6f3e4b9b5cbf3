"""The parity pin stays reproducible. tests/golden/make_golden.py regenerates the fixtures from the REFERENCE's own modules;
it recorded a SHA-256 digest of every fixture the reference produced in tests/golden/reference_digests.json, and the
committed .npz files must equal those arrays bit for bit. And the generator loads the reference's modules, not this
repo's `dpt_models` (a regular package shadows the reference's namespace package): self-referential goldens would pass
every parity test."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _digest(arrays):
    """make_golden.fixture_digest: SHA-256 over the sorted `key digest` lines, each array's digest over dtype, shape and bytes."""
    h = hashlib.sha256()
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        ha = hashlib.sha256()
        ha.update(("%s|%s|" % (a.dtype.str, a.shape)).encode())
        ha.update(a.tobytes())
        h.update(("%s %s\n" % (k, ha.hexdigest())).encode())
    return h.hexdigest()


def _stand_in_reference(root):
    """A tree shaped like the reference's dpt_models/: no __init__.py, and modules that import each other by package name."""
    pkg = os.path.join(root, "dpt_models")
    os.makedirs(pkg)
    files = {
        "embedder.py": "def get_embedder(multires, input_dims=3):\n    return None, input_dims\n",
        "fields.py": "from dpt_models.embedder import get_embedder\n\n\nclass SDFNetwork:\n    pass\n",
        "renderer.py": "import mcubes\nfrom icecream import ic\nfrom dpt_models.fields import SDFNetwork\n\n\nclass NeuSRenderer:\n    pass\n",
    }
    for name, text in files.items():
        with open(os.path.join(pkg, name), "w") as f:
            f.write(text)


def test_generator_imports_the_reference_not_this_repo(tmp_path):
    ref = os.path.realpath(str(tmp_path / "reference"))
    _stand_in_reference(ref)
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "import dpt_models.fields as mine; import make_golden as g; g.REFERENCE = %r; f, r, e = g.import_reference();"
            "assert f.__file__.startswith(%r), f.__file__;"
            "assert r.__file__.startswith(%r) and e.__file__.startswith(%r);"
            "assert f.SDFNetwork is not mine.SDFNetwork and r.SDFNetwork is f.SDFNetwork;"
            "import dpt_models.fields as again; assert again is mine; print('ok')"
            % (GOLDEN, ROOT, os.path.join(ROOT, "vdn-nerf_amd"), ref, ref + os.sep, ref + os.sep, ref + os.sep))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_committed_fixtures_are_the_references_outputs():
    want = json.load(open(os.path.join(GOLDEN, "reference_digests.json")))
    on_disk = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))
    assert sorted(want) == on_disk
    for name in on_disk:
        assert _digest(dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))) == want[name], name
