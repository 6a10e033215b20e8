import functools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


def measurement_build() -> bool:
    """True when the in-tree libraries were built with -DLEMAS_MEASUREMENT_BUILD: the kept-reproducible experiments (engine options ln_fused /
    lane_skew / xcd_runs, the LayerNorm tail of the gate + residual GEMM) exist only there; the product build refuses them."""
    from lemas_tts_amd import _lib
    return bool(_lib.testlib().lemas_k_build_flags() & 1)


MEASUREMENT_LIBDIR = os.path.join(ROOT, "lemas_tts_amd", "lib", "measurement")


def needs_measurement_build(test):
    """Measurement-only code (build() makes that pair of libraries in lemas_tts_amd/lib/measurement/): in a process holding the product
    libraries the test runs in a child pytest pointed at the measurement pair (one library pair per process: they export the same
    symbols); in a measurement process -- that child, or a tree built with -DLEMAS_MEASUREMENT_BUILD -- it runs as it is."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        if measurement_build():
            return test(*args, **kwargs)
        if not os.path.exists(os.path.join(MEASUREMENT_LIBDIR, "liblemas_hip_test.so")):
            pytest.fail("lemas_tts_amd/lib/measurement/ is missing: run build()")
        nodeid = os.environ["PYTEST_CURRENT_TEST"].rsplit(" ", 1)[0]
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", nodeid], cwd=ROOT, capture_output=True,
                           text=True, env=dict(os.environ, LEMAS_LIB_DIR=MEASUREMENT_LIBDIR))
        print(r.stdout[-3000:])
        assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return run
