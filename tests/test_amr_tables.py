"""pmc_sampler_create_mesh checks its table BEFORE any device call: every malformed table of tests/amr_checks.py is refused with
PMC_ERR_INVALID and the words that name its defect -- the same on a machine without a GPU, where a well-formed table gets as far as the
search for a device.  No GPU needed."""
import pytest

import amr_checks as A
from skirt9_amd.engine import MeshSampler


@pytest.mark.parametrize("what,tables,words", A.malformed_tables(), ids=[row[0] for row in A.malformed_tables()])
def test_a_malformed_table_is_refused_before_any_device_call(what, tables, words):
    with pytest.raises(RuntimeError, match=r"^pmc error -1: adaptive mesh: " + words + r" \(node \d\)$"):
        MeshSampler(tables, 0)


def test_missing_tables_are_refused():
    empty = {key: value[:0] for key, value in A.two_cubed().items()}
    with pytest.raises(RuntimeError, match=r"^pmc error -1: adaptive mesh tables are missing$"):
        MeshSampler(empty, 0)
