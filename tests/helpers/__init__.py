"""Helpers of the test suite. The operator registry (op_layouts.REGISTRY) is filled by op_layouts itself and by the modules listed
here, one per later family of operators: importing them with the package means that every reader of the registry --
tests/test_operator_layouts_host.py, tests/test_gpu_operator_layouts.py, run alone or with the suite -- sees all entries."""
from . import op_layouts, op_layouts_chroma  # noqa: F401
