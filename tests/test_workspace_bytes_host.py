"""CPU: the workspace sizes of the operators whose layout is stated once and measured with a null base (csrc/common.h, WsCarver):
every `chore_*_bytes` function of workspace_cases.FUNCTIONS, argument list by argument list, refused shapes (0) included.  None of
them needs a handle or a device.

The expected numbers were generated ONCE from a build of commit fd0d8c3, before the layouts were rewritten -- not from the code under
test: these byte counts are interface (callers allocate by them, launchers carve by them), so a changed number is a changed interface."""
import pytest

import workspace_cases as wc


def _lib():
    from chore_amd import _lib
    return _lib.lib


def test_every_table_is_named_and_not_empty():
    tables = {k for k, v in vars(wc).items() if k.isupper() and k != "FUNCTIONS" and isinstance(v, dict)}
    assert tables == set(wc.FUNCTIONS)
    for name in tables:
        table = getattr(wc, name)
        assert table and len({len(k) for k in table}) == 1, name
        if name not in ("GN_RELU_BWD", "HEADS_WGRAD", "CONTACT"):      # these three refuse nothing
            assert 0 in table.values() and any(table.values()), name


@pytest.mark.parametrize("name", sorted(wc.FUNCTIONS))
def test_workspace_bytes(name):
    fn, table = getattr(_lib(), wc.FUNCTIONS[name]), getattr(wc, name)
    got = {k: fn(*k) for k in table}
    assert got == table, {k: (got[k], table[k]) for k in table if got[k] != table[k]}
