"""multinerf_amd/build.py owns the list of translation units and derives the list of headers; the simulator build and the ISA
report take theirs from it.  A new kernel file is added in one place, and a new header in none."""

import glob
import os

from multinerf_amd import build
from tests.sim_helpers import tool_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_kernel_file_and_header_is_on_the_lists():
  on_disk = lambda d, *pats: sorted(p for pat in pats for p in glob.glob(os.path.join(d, pat)))
  assert sorted(build.SOURCES) == [os.path.basename(p) for p in on_disk(build.CSRC, '*.hip')]
  assert len(set(build.SOURCES)) == len(build.SOURCES) and set(build.SOURCES_F32) < set(build.SOURCES)
  assert build.HEADERS == on_disk(build.CSRC, '*.h', '*.inc') + on_disk(os.path.join(ROOT, 'include'), '*.h')
  assert os.path.join(build.CSRC, 'mesh_math.h') in build.HEADERS


def test_the_tools_take_their_lists_from_the_build():
  sim, isa = tool_module('hipsim/build.py'), tool_module('isa_report.py')
  assert sim.SOURCES is build.SOURCES and sim.SOURCES_F32 is build.SOURCES_F32
  assert set(build.HEADERS) < set(sim.DEPS) and all(os.path.exists(p) for p in sim.DEPS)
  assert list(isa.KERNEL_FILES) == [s for s in build.SOURCES if s != 'api.hip']


def test_one_pool_size(monkeypatch):
  monkeypatch.delenv('MAX_JOBS', raising=False)
  assert build.pool_size(3) == min(3, os.cpu_count()) and build.pool_size(10 ** 6) == os.cpu_count()
  monkeypatch.setenv('MAX_JOBS', '16')
  assert build.pool_size(3) == 16 and build.pool_size(10 ** 6) == 16
