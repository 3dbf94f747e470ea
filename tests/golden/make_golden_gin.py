#!/usr/bin/env python
"""Record what the reference's own configs/*.gin files bind, as this package's gin parser reads them.

    python tests/golden/make_golden_gin.py <reference checkout>     # writes tests/golden/reference_gin_bindings.json

For each file: {configurable: {parameter: repr(value)}} after `gin.parse_config_file(path, skip_unknown=True)` (the
reference's own call, internal/configs.py:185-186), so that tests/test_abi_and_config.py and tests/test_oracle_models.py
hold the shipped presets and the published parameter counts against the reference's settings without the reference at
hand (tests/helpers.py reference_gin_bindings decodes them).  `@module.fn` references are already resolved to their names
by the parser: every value is a Python literal.
"""

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OUT = os.path.join(HERE, 'reference_gin_bindings.json')
FILES = ['360', 'blender_256', 'blender_refnerf', 'llff_raw', 'blender_512', 'llff_512', 'llff_256']


def main(ref):
  from multinerf_amd import configs, gin  # noqa: F401  (importing configs registers every configurable)
  out = {}
  for name in FILES:
    gin.clear_config()
    gin.parse_config_file(os.path.join(ref, 'configs', f'{name}.gin'))
    out[name] = {t: {a: repr(v) for a, v in b.items()} for t, b in gin._BINDINGS.items()}
  gin.clear_config()
  with open(OUT, 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
  print(f'wrote {OUT}: {", ".join(FILES)}')


if __name__ == '__main__':
  if len(sys.argv) != 2:
    raise SystemExit(__doc__)
  main(sys.argv[1])
