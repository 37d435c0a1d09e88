"""The package's Python surface is pinned: every public name, every attribute
of every public class (BlockCodec's private ones included: tests and tools
call them), how each is stored (function, staticmethod, classmethod, data),
its signature and its docstring's CRC-32 equal tests/golden/python_surface.json,
which tools/python_surface.py wrote before the Python mirror was split into
the package entropy_coders_amd/fse/.  No GPU and no built library needed."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.python_surface import FIXTURE, surface  # noqa: E402


# Private methods the split added to BlockCodec when it folded repeated code:
# the only difference from the fixture, which was written before the split.
ADDED = {"BlockCodec._device_index", "BlockCodec._pack_call", "BlockCodec._pack_list", "BlockCodec._pack_compress",
         "BlockCodec._pack_decode_call", "BlockCodec._pack_selection", "BlockCodec._decompress_pack",
         "BlockCodec._decompress_pack_sealed"}


def test_surface_equals_fixture():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = json.loads(json.dumps(surface()))
    assert ADDED <= set(got) and not ADDED & set(want)
    got = {k: v for k, v in got.items() if k not in ADDED}
    assert sorted(got) == sorted(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    changed = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not changed, changed


def test_fse_is_a_package_with_the_same_names():
    import entropy_coders_amd
    from entropy_coders_amd import fse as F
    from entropy_coders_amd.fse import BlockCodec, compress2_log  # noqa: F401

    assert os.path.basename(F.__file__) == "__init__.py"
    assert len(set(F.__all__)) == len(F.__all__)
    assert set(entropy_coders_amd.__all__) == set(F.__all__) | {"FseError", "STATUS", "load"}
    for name in F.__all__:
        assert getattr(entropy_coders_amd, name) is getattr(F, name), name


def test_import_loads_neither_torch_nor_the_library():
    code = ("import sys, ctypes\n"
            "seen = []\n"
            "real = ctypes.CDLL.__init__\n"
            "def spy(self, name, *a, **k):\n"
            "    seen.append(name)\n"
            "    real(self, name, *a, **k)\n"
            "ctypes.CDLL.__init__ = spy\n"
            "import entropy_coders_amd, entropy_coders_amd.fse\n"
            "assert 'torch' not in sys.modules, 'torch was imported'\n"
            "assert not [n for n in seen if n and 'fsehip' in str(n)], seen\n"
            "print('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "clean", r.stdout + r.stderr
