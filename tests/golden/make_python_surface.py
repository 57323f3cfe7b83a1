"""The Python surface of the package, recorded: every function and class a ``labelany3d_amd/*.py`` module defines - home module,
signature, sha256 of the docstring, sha256 of the source - and the public names of the package namespace.

    python tests/golden/make_python_surface.py            # writes tests/golden/python_surface.json (run at the commit to pin)
    python tests/golden/make_python_surface.py --report   # this tree against the recording: moved, changed and absent objects

The recording was made at the commit before the Python layer was layered (``_device`` / ``segm`` / ``morph`` / ``rle_encode``) and is
committed unchanged; ``tests/test_python_surface_contract.py`` holds the tree to it.  The bare name is the key: at the recording every
name was unique across the modules (the maker refuses to write otherwise)."""
import hashlib
import importlib
import inspect
import json
import os
import pkgutil
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATH = os.path.join(HERE, "python_surface.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _sha(text) -> str:
    return hashlib.sha256((text or "").encode()).hexdigest()


def _signature(obj) -> str:
    try:
        # (a sentinel default prints its address, a path default the place of the checkout)
        return re.sub(r" at 0x[0-9a-f]+", "", str(inspect.signature(obj))).replace(ROOT, "<root>")
    except ValueError:   # (a ctypes structure has none: its fields stand in)
        return "(" + ", ".join(f[0] for f in getattr(obj, "_fields_", ())) + ")"


def modules():
    """The ``labelany3d_amd/*.py`` modules (no subpackages), imported, by name."""
    import labelany3d_amd

    names = sorted(m.name for m in pkgutil.iter_modules(labelany3d_amd.__path__) if not m.ispkg)
    return {n: importlib.import_module("labelany3d_amd." + n) for n in names}


def surface() -> dict:
    """-> {"objects": {bare name: {module, signature, doc, source}}, "public": [names of the package namespace]}"""
    import labelany3d_amd

    objects, twice = {}, []
    for mod_name, mod in modules().items():
        for name, obj in vars(mod).items():
            if not (inspect.isfunction(obj) or inspect.isclass(obj)) or obj.__module__ != mod.__name__ or obj.__name__ != name:
                continue
            if name in objects:
                twice.append(name)
            objects[name] = dict(module=mod_name, signature=_signature(obj), doc=_sha(inspect.getdoc(obj)),
                                 source=_sha(inspect.getsource(obj)))
    if twice:
        raise SystemExit(f"defined in more than one module, so the bare name is no key: {sorted(twice)}")
    public = sorted(n for n, v in vars(labelany3d_amd).items() if not n.startswith("_") and not inspect.ismodule(v))
    return dict(objects=dict(sorted(objects.items())), public=public)


def report(pinned: dict, now: dict) -> dict:
    """What differs between the recording and this tree -> {"moved": {name: [from, to]}, "changed_source": [...], "changed_signature":
    [...], "changed_doc": [...], "absent": [...], "new": [...], "public_lost": [...]}"""
    was, has = pinned["objects"], now["objects"]
    both = [n for n in was if n in has]
    return dict(moved={n: [was[n]["module"], has[n]["module"]] for n in both if was[n]["module"] != has[n]["module"]},
                changed_source=[n for n in both if was[n]["source"] != has[n]["source"]],
                changed_signature=[n for n in both if was[n]["signature"] != has[n]["signature"]],
                changed_doc=[n for n in both if was[n]["doc"] != has[n]["doc"]],
                absent=[n for n in was if n not in has], new=[n for n in has if n not in was],
                public_lost=[n for n in pinned["public"] if n not in now["public"]])


if __name__ == "__main__":
    if "--report" in sys.argv[1:]:
        with open(PATH) as fh:
            print(json.dumps(report(json.load(fh), surface()), indent=1))
    else:
        s = surface()
        with open(PATH, "w") as fh:
            fh.write(json.dumps(s, indent=1) + "\n")
        print(f"{len(s['objects'])} objects, {len(s['public'])} public names -> {PATH}")
