"""The reference's OWN scan registration (scanRegistration.cpp), compiled unchanged against declared container doubles.

TEST INFRASTRUCTURE ONLY, like orc.py.  build() is the recipe: it compiles the reference's source file where it lies
(nothing of it is copied into this tree) with the reference's own flags (CMakeLists.txt:4-6: -std=c++14 -O3 -g, no
-march, no fast-math), `main` renamed, against oracle/ref_standins/ (PCL containers, message conversions, a recording
pass-through VoxelGrid) and tests/native/ros_double/ (roscpp, messages), and links it with oracle/ref_driver.cpp into
oracle/_ref/ (kept out of git).  Two variants:

    scanreg_f32   -include math.h: the unqualified atan / sqrt of scanRegistration.cpp:139 bind to the float overloads
                  (assumption A1 of DESIGN section 6; what the oracle and k_organize implement)
    scanreg_f64   as written: with <cmath> alone they bind to ::atan / ::sqrt (double)

Where the reference directory does not exist, build() does nothing and whatever is already in oracle/_ref/ is used.
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
REF_ROOT = os.environ.get("LIGHTLOAM_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(_HERE, "_ref")
VARIANTS = {"f32": ["-include", "math.h"], "f64": []}
CXXFLAGS = ["-std=c++14", "-O3", "-g"]
MAIN = "ll_ref_scan_registration_main"
MAX_POINTS = 400000          # the reference's fixed arrays (scanRegistration.cpp:34-40); it checks nothing


def _source():
    return os.path.join(REF_ROOT, "src", "scanRegistration.cpp")


def reference_present():
    return os.path.isfile(_source())


def binary(variant):
    return os.path.join(OUT, "scanreg_" + variant)


def available(variant="f32"):
    return os.path.isfile(binary(variant)) and os.access(binary(variant), os.X_OK)


def _recipe_inputs():
    deps = [os.path.abspath(__file__), os.path.join(_HERE, "ref_driver.cpp")]
    for d in (os.path.join(_HERE, "ref_standins"), os.path.join(_ROOT, "tests", "native", "ros_double")):
        for base, _, files in os.walk(d):
            deps += [os.path.join(base, f) for f in files]
    return deps


def build(force=False):
    """Builds both variants into oracle/_ref/ when the reference is there and they are missing or older than the recipe,
    the doubles, the driver or the reference's source.  Returns the list of binaries that exist afterwards.

    Several processes may call this at once (the ranks of tests/test_distributed_gloo.py, two test runs over one tree): one
    builds under a file lock while the others wait and then find the binaries fresh; every build works in a directory of its
    own and a finished binary takes its place in one rename, so that nobody ever runs or links a half-written file."""
    if reference_present():
        import fcntl
        inc = ["-I", os.path.join(_HERE, "ref_standins"), "-I", os.path.join(_ROOT, "tests", "native", "ros_double")]
        newest = max(os.path.getmtime(p) for p in _recipe_inputs() + [_source()])
        cxx = os.environ.get("CXX", "g++")

        def fresh(variant):
            return not force and os.path.isfile(binary(variant)) and os.path.getmtime(binary(variant)) >= newest

        if all(fresh(v) for v in VARIANTS):                     # nothing to write: a read-only tree is fine
            return [binary(v) for v in VARIANTS if available(v)]
        os.makedirs(OUT, exist_ok=True)
        with open(os.path.join(OUT, ".lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)                    # released when the file is closed
            for variant, extra in VARIANTS.items():
                exe = binary(variant)
                if fresh(variant):                              # built while this process waited for the lock
                    continue
                with tempfile.TemporaryDirectory(prefix="build_", dir=OUT) as work:
                    obj, tmp = os.path.join(work, f"scanreg_{variant}.o"), os.path.join(work, "scanreg_" + variant)
                    subprocess.check_call([cxx] + CXXFLAGS + extra + ["-D", "main=" + MAIN] + inc +
                                          ["-I", os.path.join(REF_ROOT, "include"), "-c", _source(), "-o", obj])
                    subprocess.check_call([cxx] + CXXFLAGS + inc + [os.path.join(_HERE, "ref_driver.cpp"), obj, "-o", tmp])
                    os.replace(tmp, exe)
    return [binary(v) for v in VARIANTS if available(v)]


def ring_of(points):
    """Ring of published points from their intensity = scanID + 0.1 * relTime (scanRegistration.cpp:208).  relTime lies in
    [-0.5, 1.5] (:177-207), so the ring is the NEAREST integer; it is int(intensity) wherever relTime >= 0 (a point just
    before the start azimuth has relTime < 0 and int() would read the ring below, tests/test_oracle.py)."""
    return np.rint(np.asarray(points, np.float32).reshape(-1, 4)[:, 3]).astype(np.int32)


def scan_bounds(cloud, rings):
    """scanStartInd / scanEndInd of :216-221 (locals of the handler) from laserCloud, which is the rings in ascending order"""
    ring = ring_of(cloud)
    assert (np.diff(ring) >= 0).all() and (len(ring) == 0 or (ring[0] >= 0 and ring[-1] < rings)), "laserCloud is not ring-ordered"
    count = np.bincount(ring, minlength=rings)
    end = np.cumsum(count)
    return (end - count + 5).astype(np.int32), (end - 6).astype(np.int32)


def _pack(scans):
    scans = [np.ascontiguousarray(s, dtype=np.float32) for s in scans]
    stride = scans[0].shape[1]
    assert stride in (3, 4) and all(s.ndim == 2 and s.shape[1] == stride for s in scans), "scans of one call share one point size"
    assert all(0 < len(s) <= MAX_POINTS for s in scans), "the reference indexes points[0] and 400 000-element arrays unchecked"
    parts = [struct.pack("<ii", len(scans), stride)]
    for s in scans:
        parts += [struct.pack("<i", len(s)), s.tobytes()]
    return b"".join(parts)


def _unpack(buf, rings):
    off = 0

    def take(dtype, count, width=1):
        nonlocal off
        a = np.frombuffer(buf, dtype=dtype, count=count * width, offset=off).copy()
        off += a.nbytes
        return a.reshape(count, width) if width > 1 else a

    out = []
    for _ in range(int(take("<i4", 1)[0])):
        n, ns, nls, nf, nv = (int(v) for v in take("<i4", 5))
        r = dict(rc=0, cloud=take("<f4", n, 4), sharp=take("<f4", ns, 4), less_sharp=take("<f4", nls, 4), flat=take("<f4", nf, 4),
                 curv=take("<f4", n), label=take("<i4", n))
        r["voxel_inputs"] = [take("<f4", int(take("<i4", 1)[0]), 4) for _ in range(nv)]
        r["scan_start"], r["scan_end"] = scan_bounds(r["cloud"], rings)
        out.append(r)
    assert off == len(buf), "trailing bytes in the reference driver's output"
    return out


def extract(scans, rings, minimum_range, variant="f32", lower_bound=-24.9, up_bound=2.0):
    """scans: list of (n, 3) or (n, 4) float32 arrays (12- or 16-byte input points), handed IN ORDER to the laser-cloud
    callback of ONE reference process.  Returns one dict per scan with orc.extract's keys where they exist -- cloud, curv,
    label (both meaningful on [5, n-5) only: the rest is whatever earlier scans left in the reference's globals),
    scan_start, scan_end (recomputed, see scan_bounds), sharp, less_sharp, flat -- plus voxel_inputs: the clouds the
    reference handed to VoxelGrid::filter, one per non-skipped ring in ring order.  There is no less_flat: see
    ref_standins/pcl/filters/voxel_grid.h.  Every scan must be non-empty after the reference's filtering."""
    if not available(variant):
        raise RuntimeError(f"{binary(variant)} is missing: oracle.ref.build() needs the reference tree at {REF_ROOT}")
    with tempfile.TemporaryDirectory(prefix="ll_ref_") as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(_pack(scans))
        p = subprocess.run([binary(variant), fin, fout, str(int(rings)), repr(float(minimum_range)), repr(float(lower_bound)), repr(float(up_bound))],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"{binary(variant)} exited with {p.returncode}: {p.stderr.decode(errors='replace')[-500:]}")
        with open(fout, "rb") as f:
            buf = f.read()
    out = _unpack(buf, rings)
    assert len(out) == len(scans)
    return out
