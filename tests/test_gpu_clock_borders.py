"""tests/test_gpu_borders.py for the step-count extension: every case of tests/clock_abi_cases.py between poisoned borders
(a plain run, an arena run per fill; outputs bit-identical, borders and inputs untouched), then what the extension's row of
tests/borders.TABLE asserts of the plain run; and that every export of ``_lib.CLOCK_SIGNATURES`` has a case or a reason.  GPU only;
no tolerance anywhere."""
from borders import completeness_test, ctx, export_test  # noqa: F401  (ctx: the module's fixture)

test_clock_export_between_poisoned_borders = export_test('clock')
test_every_clock_export_has_a_case = completeness_test('clock')
