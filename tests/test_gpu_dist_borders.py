"""tests/test_gpu_borders.py for the data-parallel extension: every case of tests/dist_abi_cases.py between poisoned borders
(a plain run, an arena run per fill; outputs bit-identical, borders and inputs untouched), then what the extension's row of
tests/borders.TABLE asserts of the plain run; and that every export of ``_lib.DIST_SIGNATURES`` has a case or a reason.  GPU only;
no tolerance anywhere."""
import pytest

from borders import completeness_test, ctx, export_test  # noqa: F401  (ctx: the module's fixture)

test_dist_export_between_poisoned_borders = export_test('dist')
test_every_dist_export_has_a_case = completeness_test('dist')


@pytest.mark.gpu
def test_argument_checks_and_the_empty_table(ctx):
    """check_table's pattern: -1 with a message for negative counts, a null table and chunks without tensors; no chunks is a no-op"""
    lib, st = ctx.lib, ctx.stream()
    assert lib.dcf_dist_pack_grads(None, None, 0, 0, 0.5, st) == 0
    assert lib.dcf_dist_pack_grads(None, None, 3, 0, 0.5, st) == 0
    for args, word in (((None, None, 1, 1), 'null table'), ((None, None, -1, 0), 'negative'), ((None, None, 1, -1), 'negative'),
                       ((None, None, 1, 1 << 31), 'exceed')):
        assert lib.dcf_dist_pack_grads(*args, 0.5, st) == -1
        msg = lib.dcf_last_error().decode()
        assert 'dcf_dist_pack_grads' in msg and word in msg, msg
