"""tests/test_gpu_project.py and tests/test_gpu_tsdf_cameras.py run on the kernel-source simulator in a child pytest
(MNR_TESTS_ON_SIMULATOR=1, the way tests/test_sim_tsdf.py runs its file): the forward camera model of csrc/camera_project.h in
mnr_project_points and in the general fusion kernel of csrc/tsdf.hip (the staging of the records, the per-brick culling by model and
its ballot compaction, the launches of a stack longer than one launch stages) against the NumPy restatement, with the test code
unchanged.  The model and the script are left to the MI355X: they run no kernel of these files' subject that the other tests do
not."""

import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not (shutil.which('clang++') or os.path.exists('/opt/rocm/lib/llvm/bin/clang++')),
                                reason='needs clang++')


def test_camera_projection_kernels_pass_on_the_simulator():
  env = dict(os.environ, MNR_TESTS_ON_SIMULATOR='1')
  cmd = [sys.executable, '-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_gpu_project.py',
         'tests/test_gpu_tsdf_cameras.py', '-k', 'not script and not renders']
  r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
  tail = '\n'.join((r.stdout + r.stderr).splitlines()[-25:])
  assert r.returncode == 0, tail
  assert ' passed' in tail and 'failed' not in tail and 'skipped' not in tail, tail
