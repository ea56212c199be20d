"""CPU: the surface of 3dbodyanimation_amd.torch_layer is what tests/golden/torch_layer_surface.json recorded: every public name
(no leading underscore, defined in the layer and not imported into it) is there, and every function, and every class's __init__ /
forward / evaluate / normal_equations where the layer defines one, has the recorded signature; so are the private names the tests
and the tools reach.

The fixture was written by running this file (python tests/test_torch_layer_surface.py) at the commit BEFORE the layer's repeated
code was folded into shared helpers and torch_layer.py became a package, from the single module; it is regenerated only when
the surface changes on purpose."""
import importlib
import inspect
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "torch_layer_surface.json")
METHODS = ("__init__", "forward", "evaluate", "normal_equations")
PRIVATE = ("_raster_handle", "_surface_handle", "_render", "_SignedRoot")


def _own(tl, obj) -> bool:
    """defined in the layer (the module, or a module of the package), not imported into it"""
    m = getattr(obj, "__module__", None)
    return isinstance(m, str) and (m == tl.__name__ or m.startswith(tl.__name__ + "."))


def surface(tl) -> dict:
    out = {}
    for name in sorted(n for n in vars(tl) if not n.startswith("_")):
        obj = getattr(tl, name)
        if not _own(tl, obj) or not (inspect.isfunction(obj) or inspect.isclass(obj)):
            continue
        if inspect.isfunction(obj):
            out[name] = str(inspect.signature(obj))
            continue
        for m in METHODS:
            if any(m in vars(k) for k in obj.__mro__ if _own(tl, k)):
                out[f"{name}.{m}"] = str(inspect.signature(getattr(obj, m)))
        out.setdefault(name, "class")
    return out


def test_every_recorded_name_is_there_with_its_signature():
    tl = importlib.import_module("3dbodyanimation_amd.torch_layer")
    want = json.load(open(GOLDEN))
    assert len(want["names"]) >= 30 and set(want["names"]) <= set(want["signatures"])
    got = surface(tl)
    for name in want["names"]:
        assert hasattr(tl, name), name
    assert sorted(k for k in got if "." not in k) == want["names"]       # (and no public name that was not there)
    for key, sig in want["signatures"].items():
        assert got.get(key) == sig, f"{key}: {got.get(key)} is not the recorded {sig}"
    for name in PRIVATE:
        assert hasattr(tl, name), name


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    sig = surface(importlib.import_module("3dbodyanimation_amd.torch_layer"))
    json.dump({"names": sorted(k for k in sig if "." not in k), "signatures": sig}, open(GOLDEN, "w"), indent=1, sort_keys=True)
    print(len(sig), "entries ->", GOLDEN)
