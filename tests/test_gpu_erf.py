"""ok_erff compiled for the device: the same bits as the host compilation on the whole set of tests/test_erf_rule.py."""
import numpy as np
import pytest

import _erf_cases as E
import _math_cases as M

pytestmark = pytest.mark.gpu


def test_device_equals_host(gpu):
    a = E.erf_set()
    dev, host = E.evaluate(gpu, 0), E.evaluate(gpu, M.ON_HOST)
    finite = a == a
    M.assert_same_bits("erf, device against host", dev[finite], host[finite], a[finite])
    assert np.isnan(dev[~finite]).all()
