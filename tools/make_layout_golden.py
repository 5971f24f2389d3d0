"""tests/golden/layout_contract.json: the sizes and offsets tests/test_layout_contract.py compares against,
asked of a library built from the commit BEFORE the change under test (never of the tree's own build):

    git stash / checkout the parent; python -c "import __graft_entry__ as g; g.build()"
    cp polymer-chemprop_amd/chemprop_amd/libwdmpnn.so /tmp/parent.so; return to the change
    WDMPNN_LIB=/tmp/parent.so PYTHONDONTWRITEBYTECODE=1 python tools/make_layout_golden.py

The table of cases and the queries are the test module's own (cases, query)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'polymer-chemprop_amd')]

from chemprop_amd import _native  # noqa: E402

import test_layout_contract as T  # noqa: E402


def main():
    if 'WDMPNN_LIB' not in os.environ:
        sys.exit('set WDMPNN_LIB to the parent commit\'s library: the golden file is not made from the code under test')
    L = _native.lib()
    out = {}
    for kind, n, msg in T.GROUPS:
        for case in T.cases(kind, n, msg):
            out[case[0]] = T.query(L, kind, n, msg, case)
    with open(T.GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in out.items()) + '\n}\n')
    print('wrote', T.GOLDEN, len(out), 'cases,', sum('rc' in v for v in out.values()), 'refused, library', _native.LIB_PATH)


if __name__ == '__main__':
    main()
