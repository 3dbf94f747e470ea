"""tests/test_gpu_ingest.py run on the kernel-source simulator in a child pytest (MNR_TESTS_ON_SIMULATOR=1, the way
tests/test_sim_raw.py runs its file): mnr_image_ingest's three kernels (flat, per pixel, strips through LDS) against the
NumPy float32 restatements, the argument errors, the Blender / LLFF / Tanks and Temples loaders on the "device" against the
host path, with the test code unchanged.  The two train steps of the `360+tat` preset are left to the MI355X: 1024 rays
through the whole model take the simulator the better part of an hour, and they run no kernel of this file's subject."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_ingest_kernels_and_loaders_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_ingest.py', '-k', 'not two_train_steps']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
