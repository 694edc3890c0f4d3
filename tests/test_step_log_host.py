"""Host side of the step log (include/srbm_rti.h: srbm_step_log_*), without a GPU: the record size the library reports, the field table of
host.py, and the statistics row made from a record.  What the records hold is tested on the device (tests/test_gpu_step_log.py)."""
import ctypes
import io

import numpy as np
import pytest

from srbm_loader import host


@pytest.fixture(scope='module')
def libpath():
    return host.build()


def test_record_size_is_reported_without_a_gpu(libpath):
    for path in (libpath, host.LIB_PATH_LARGE):
        assert ctypes.CDLL(path).srbm_step_log_record_doubles() == 64
    assert host.STEP_LOG_DOUBLES == 64


def test_field_table_tiles_the_record():
    """the named fields cover [0, 58) once each; [58, 64) is reserved"""
    covered = np.zeros(host.STEP_LOG_DOUBLES, int)
    for name, sl in host.STEP_LOG_FIELDS.items():
        assert sl.step is None and 0 <= sl.start < sl.stop <= 58, (name, sl)
        covered[sl] += 1
    assert covered[:58].tolist() == [1] * 58 and not covered[58:].any()
    widths = {k: v.stop - v.start for k, v in host.STEP_LOG_FIELDS.items()}
    assert (widths['stats'], widths['state'], widths['ee'], widths['force'], widths['in_contact']) == (8, 13, 12, 12, 4)
    assert (host.STEP_LOG_FIELDS['stats'].start, host.STEP_LOG_FIELDS['state'].start, host.STEP_LOG_FIELDS['force'].start) == (7, 17, 42)


def test_stat_line_from_a_record_is_the_shared_formatter_on_its_values():
    rng = np.random.default_rng(11)
    r = rng.normal(size=host.STEP_LOG_DOUBLES)
    r[0], r[2] = 17, 1                                       # solve number, status 'Solved Inacc'
    stats = r[7:15].copy()                                   # alpha, cost, defect, step norm, iterations, residuals, gap
    merit = stats[1] + 5000.0 * stats[2]                     # srbm_get_merit: cost + mu * defect
    buf = io.StringIO()
    host.stat_line_from_log(buf, r, 3.5)
    want = host.format_stat_line(17, 3.5, stats, merit, r[16], 1)
    assert buf.getvalue() == want
    cols = [want[i:i + 15] for i in range(0, 150, 15)]
    assert want.endswith('\n') and len(want) == 151
    assert cols[0].strip() == '17' and cols[1].strip() == '3.5' and cols[8].strip() == 'Solved Inacc'
    assert cols[2].strip() == '%g' % stats[2] and cols[5].strip() == '%g' % stats[1] == cols[9].strip() and cols[6].strip() == '%g' % merit
    assert host.step_log_merit(r) == merit and host.step_log_merit(np.stack([r, r])).shape == (2,)
    r[2] = 42
    buf = io.StringIO(); host.stat_line_from_log(buf, r, 0.0)
    assert buf.getvalue()[120:135].strip() == 'Other'
