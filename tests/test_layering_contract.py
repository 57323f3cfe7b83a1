"""CPU-only, AST-only (nothing of the package is imported): the modules of ``labelany3d_amd`` import one way.  ``RANKS`` is the order of
the package, one rank per row: a module imports only from modules of a strictly LOWER rank - at any depth, function-level imports
included; modules of one row do not import each other -, keeps its
module-level imports above its first ``def`` / ``class``, and takes every name from the module that defines it, never through a third
one.  The two facades (``masks``, ``__init__``) re-export by design and are not asked where their names come from; ``batched`` imports
the ``_device`` names it hands on to old callers (``batched._upload_many``), which nothing here forbids - but no module of the package
may take them THROUGH it."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "labelany3d_amd")

RANKS = (("_build",),                      # (the build recipe; ``_lib`` loads what it builds, so it stands below ``_lib``)
         ("_lib", "options"),
         ("_device",),
         ("segm",),
         ("batched",),
         ("fitcall",),
         ("bits",),
         ("labels", "depth16"),
         ("frames",),
         ("morph", "rle_encode", "components", "overlap", "clouds"),
         ("assign",),
         ("consumers", "depth_align", "jsonout", "ply"),
         ("masks",),
         ("pipeline", "shard", "fit_scenes", "combine", "util", "util_3dbox", "cam_utils"),
         ("compat", "__init__"))
RANK = {name: i for i, row in enumerate(RANKS) for name in row}
FACADES = ("masks", "__init__")                 # they import names in order to pass them on


def _modules():
    out = {}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        with open(path) as fh:
            out[os.path.basename(path)[:-3]] = ast.parse(fh.read(), path)
    return out


def _targets(node):
    """the package modules an import statement reaches, as (module, [names taken from it] or None for the module itself)"""
    if isinstance(node, ast.ImportFrom):
        if node.level == 1 and node.module is None:                       # from . import _lib, options
            return [(a.name, None) for a in node.names]
        if node.level == 1:                                               # from .bits import MaskBits
            return [(node.module.split(".")[0], [a.name for a in node.names])]
        if node.level == 0 and node.module and (node.module + ".").startswith("labelany3d_amd."):   # (``from labelany3d_amd import x`` too)
            rest = node.module.split(".")[1:]
            return [(rest[0], [a.name for a in node.names])] if rest else [(a.name, None) for a in node.names]
        assert node.level <= 1, "an import that climbs out of the package"
    elif isinstance(node, ast.Import):
        # (a bare ``import labelany3d_amd`` reaches the package itself: the top of the order)
        return [((a.name.split(".") + ["__init__"])[1], None) for a in node.names if (a.name + ".").startswith("labelany3d_amd.")]
    return []


def _defined(tree):
    """the names a module's own statements define or assign at module scope (imports do not count)"""
    names = set()

    def visit(body):
        for node in body:
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                names.add(node.name)
                continue
            if isinstance(node, (ast.Import, ast.ImportFrom)):
                continue
            for sub in ast.walk(node):
                if isinstance(sub, ast.Name) and isinstance(sub.ctx, ast.Store):
                    names.add(sub.id)
    visit(tree.body)
    return names


def _module_level(body):
    """the statements that run when the module is imported: its body, and what ``if`` / ``try`` / ``with`` / loops nest in it"""
    for node in body:
        yield node
        if not isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            for field in ("body", "orelse", "finalbody"):
                yield from _module_level(getattr(node, field, []) or [])
            for handler in getattr(node, "handlers", []):
                yield from _module_level(handler.body)


def test_every_module_has_a_rank():
    mods, placed = _modules(), [name for row in RANKS for name in row]
    assert sorted(set(mods) - set(placed)) == [], "a module of the package that the table does not place"
    assert sorted(set(placed) - set(mods) - {"compat"}) == [], "the table names a module that is gone"
    assert len(set(placed)) == len(placed)


def test_imports_run_one_way():
    bad = []
    for name, tree in _modules().items():
        for node in ast.walk(tree):
            for target, _ in _targets(node):
                if target not in RANK:
                    bad.append(f"{name}.py:{node.lineno} imports {target}, which the table does not place")
                elif RANK[target] >= RANK[name]:
                    bad.append(f"{name}.py:{node.lineno} imports {target}, whose rank is not lower")
    assert bad == []


def test_module_level_imports_stand_above_the_first_definition():
    bad = []
    for name, tree in _modules().items():
        if name == "__init__":
            continue
        level = list(_module_level(tree.body))
        first = min((n.lineno for n in level if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef))), default=None)
        if first is not None:
            bad += [f"{name}.py:{n.lineno}" for n in level if isinstance(n, (ast.Import, ast.ImportFrom)) and n.lineno > first]
    assert bad == []


def test_names_come_from_the_module_that_defines_them():
    mods = _modules()
    defined = {name: _defined(tree) for name, tree in mods.items()}
    bad = []
    for name, tree in mods.items():
        if name in FACADES:
            continue
        for node in ast.walk(tree):
            for target, taken in _targets(node):
                if taken is None or target not in defined:
                    continue
                bad += [f"{name}.py:{node.lineno} takes {t} from {target}, which does not define it" for t in taken if t not in defined[target]]
    assert bad == []


def test_masks_has_no_late_imports():
    with open(os.path.join(PKG, "masks.py")) as fh:
        assert "noqa: E402" not in fh.read()
