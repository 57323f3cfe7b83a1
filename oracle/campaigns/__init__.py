"""The differential campaigns: case generators, oracle runners, GPU runners and the per-run checkers that profiles/r06/fuzz_*.py
(the campaigns at scale) and tests/test_gpu_differential.py (committed slices of their seeds, tests/campaign_slices.py) share.
Test infrastructure, like the rest of this package; the checkers hold records to tests/test_gpu_parity.py::assert_records' rule."""
