"""The rule that keeps the test modules independent of each other: nothing under tests/ or tools/ imports from a test module.
What two of them need lives in tests/suite_support.py, tests/ref_build.py or tools/cost_common.py.  No GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPORT_OF_A_TEST_MODULE = re.compile(r"^\s*(?:from|import)\s+(?:[\w.]*\.)?test_\w*", re.M)


def test_nothing_imports_from_a_test_module():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    assert len(files) > 60, "the sources were found"
    found = [f"{os.path.relpath(f, ROOT)}: {m.group(0).strip()}" for f in files for m in IMPORT_OF_A_TEST_MODULE.finditer(open(f).read())]
    assert not found, found
