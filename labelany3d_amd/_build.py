"""Build recipe of libla3d.so — importable by file path without importing the package (which loads
the library and fails loudly when it is missing)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
# one translation unit per engine (compiled side by side), the C-ABI + dispatcher, the other kernels, the host-side JSON writer (last:
# it carries the build identity)
# (la3d_instance_f16.hip / la3d_instance_u16.hip: la3d_instance.hip once more for the 16-bit depth planes, each a unit of its own)
# (la3d_hull_finish.hip: the kernels behind the fit kernel of a convex-hull call - they read no depth, so they are compiled once, not
# with each of the three instance units)
# (la3d_cloud.hip: the instance point clouds, kernels and C entries in one unit)
# (la3d_bits.hip: the packers of bit planes, the unpacker, the plane statistics and the annotation decoders)
# (la3d_rle_encode.hip: bit planes -> COCO run lengths, kernels and C entries in one unit)
# (la3d_open.hip: binary opening on bit planes, uniform and frames form, kernels and C entries in one unit)
# (la3d_components.hip: connected components on bit planes - largest part, island removal -, uniform and frames form, kernel and C entries in one unit)
# (la3d_bitplanes.hpp: what those four share - BitsOut, the frames prologue, the plane locator of a frames call that reads and writes planes
# (FramesPlanes), the row word, pack_check, the in-place rule -; la3d_cloud.hip takes its prologue, la3d_overlap.hip its at() and offset rule)
# (la3d_align.hip: the batched RANSAC scale fit of the depth alignment, kernels and C entries in one unit)
# (la3d_overlap.hip: pairwise mask overlap on bit planes and the mask NMS that reads it, kernels and C entries in one unit)
# (la3d_assign.hip: the batched linear sum assignment that reads an overlap or IoU matrix, kernel and C entry in one unit)
# (la3d_depth_gate.hip: the depth gate on bit planes - a mask's depth outliers dropped before the fit -, kernel and C entry in one unit;
# la3d_select.hpp: the exact median under a bit image, which it shares with la3d_consumers.hip)
# (la3d_plane.hip: the ground plane from the depth - sample select and batched RANSAC plane fit -, kernels and C entries in one unit;
# la3d_point.hpp: the back-projected pixel it shares with la3d_cloud.hip; la3d_draw.hpp: the device draw it shares with la3d_align.hip)
SOURCES = [os.path.join(CSRC, f) for f in ("la3d_instance.hip", "la3d_instance_f16.hip", "la3d_instance_u16.hip", "la3d_hull_finish.hip", "la3d_band.hip", "la3d_rows.hip", "la3d_split.hip", "la3d_points.hip", "la3d_masks.hip", "la3d_bits.hip", "la3d_rle_encode.hip", "la3d_open.hip", "la3d_components.hip", "la3d_depth16.hip", "la3d_consumers.hip", "la3d_cloud.hip", "la3d_align.hip", "la3d_overlap.hip", "la3d_assign.hip", "la3d_depth_gate.hip", "la3d_plane.hip", "la3d.hip",
                                           "la3d_json.cpp")]
HEADERS = [os.path.join(CSRC, f) for f in ("la3d_device.hpp", "la3d_walks.hpp", "la3d_stages.hpp", "la3d_instance_phases.hpp", "la3d_engines.hpp", "la3d_poly.hpp", "la3d_hull.hpp", "la3d_bitplanes.hpp", "la3d_select.hpp", "la3d_point.hpp", "la3d_draw.hpp")] + \
          [os.path.join(ROOT, "include", "la3d.h")]
LIB = os.environ.get("LA3D_LIB") or os.path.join(HERE, "lib", "libla3d.so")  # LA3D_LIB: experiment builds only
INCLUDE = os.path.join(ROOT, "include")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"]


def source_sha256() -> str:
    """Hash of everything libla3d.so is compiled from (sources and headers, fixed order, names included)."""
    import hashlib
    h = hashlib.sha256()
    for f in SOURCES + HEADERS:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()


def compile_cmd_sha256() -> str:
    """Hash of the compile command: the flags and the compiler's own version line."""
    import hashlib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    try:
        ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    except Exception:  # noqa: BLE001
        ver = "unknown"
    return hashlib.sha256((" ".join(HIPCC_FLAGS) + "|" + ver).encode()).hexdigest()


def embedded_info(lib_path: str = LIB):
    """(sources hash, compile-command hash) the library at lib_path was built from - read from the file's bytes (the string
    la3d_build_info() returns), without loading it - or None for a library that carries none."""
    import re
    try:
        data = open(lib_path, "rb").read()
    except OSError:
        return None
    m = re.search(rb"LA3D_BUILD_INFO:([0-9a-f]{64}):([0-9a-f]{64})", data)
    return (m.group(1).decode(), m.group(2).decode()) if m else None


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the sources of csrc/ for gfx950 into lib/libla3d.so (in-tree, so it travels with the repo): one object per
    translation unit, compiled side by side, then one link.  The hash of the sources and of the compile command is compiled INTO
    the library (la3d_build_info); an existing library is reused only when the hash it carries is the hash of the tree's sources
    (not by file time: a library that travelled with a snapshot proves what it was built from)."""
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    src_hash = source_sha256()
    if not force and os.path.exists(LIB):
        have = embedded_info(LIB)
        if have is not None and have[0] == src_hash:
            if verbose:
                print(f"libla3d.so is current: built from sources sha256 {src_hash[:16]}.. (compile command {have[1][:16]}..)")
            return LIB
    import tempfile
    from concurrent.futures import ThreadPoolExecutor

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd_hash = compile_cmd_sha256()
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]
    with tempfile.TemporaryDirectory(prefix="la3d_build_") as tmp:
        objs = [os.path.join(tmp, os.path.splitext(os.path.basename(src))[0] + ".o") for src in SOURCES]
        cmds = [[hipcc, *flags, "-I", INCLUDE, "-c", src, "-o", obj] for src, obj in zip(SOURCES, objs)]
        # the host-only translation unit carries the identity string
        cmds[-1][1:1] = [f'-DLA3D_BUILD_SOURCES="{src_hash}"', f'-DLA3D_BUILD_CMD="{cmd_hash}"']
        if verbose:
            for c in cmds:
                print(" ".join(c))
        with ThreadPoolExecutor(max_workers=len(cmds)) as ex:
            for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds):
                if r.returncode != 0:
                    raise RuntimeError("hipcc failed:\n" + r.stderr[-4000:])
        link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
        if verbose:
            print(" ".join(link))
        subprocess.run(link, check=True)
    if verbose:
        print(f"libla3d.so built from sources sha256 {src_hash[:16]}.. with compile command {cmd_hash[:16]}..")
    assert embedded_info(LIB) == (src_hash, cmd_hash), "the library does not carry the identity it was built with"
    return LIB


EXAMPLE_SRC = os.path.join(ROOT, "examples", "fit_from_c.cpp")
EXAMPLE_BIN = os.path.join(HERE, "lib", "fit_from_c")


def build_example(force: bool = False, verbose: bool = False) -> str:
    """The plain host program that drives the C-ABI without Python (examples/fit_from_c.cpp), linked against the in-tree
    library; tests/test_gpu_cabi.py runs it on the GPU box."""
    lib = build(force=False, verbose=verbose)
    if not force and os.path.exists(EXAMPLE_BIN) and os.path.getmtime(EXAMPLE_BIN) >= max(os.path.getmtime(EXAMPLE_SRC),
                                                                                         os.path.getmtime(lib)):
        return EXAMPLE_BIN
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O2", "-std=c++17", "-I", INCLUDE, EXAMPLE_SRC, "-L", os.path.dirname(lib), "-lla3d", "-Wl,-rpath,$ORIGIN",
           "-o", EXAMPLE_BIN]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return EXAMPLE_BIN


