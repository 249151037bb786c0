"""The one Python path of the exclusion lists, without a GPU: ``ops.exclusions_on_device`` on device "cpu" (what every call that takes
`exclude` sends to the library) and ``recommender._exclusion_lists`` (dict or aligned list -> one list per user)."""
import numpy as np
import pytest
import torch

from foodrec_amd.ops import exclusion_csr, exclusions_on_device
from foodrec_amd.recommender import _exclusion_lists

LISTS = [[4, 2, 4], [], [9, 0, 7, 7], [3]]
CALLERS = (("topk_users_excluding", ValueError), ("topk_users_mlp_excluding", ValueError), ("catalogue_rank", ValueError),
           ("topk_markets_excluding", TypeError))                # (what, what a wrong dtype of a device pair raises there)


def _same(got, want):
    off, ids = got
    assert off.dtype == torch.int64 and ids.dtype == torch.int32 and off.device.type == ids.device.type == "cpu"
    assert off.tolist() == want[0].tolist() and ids.tolist() == want[1].tolist()


def test_lists_and_host_pairs_are_exclusion_csr():
    want = exclusion_csr(LISTS, 4)
    assert want[0].tolist() == [0, 2, 2, 5, 6] and want[1].tolist() == [2, 4, 0, 7, 9, 3]
    _same(exclusions_on_device(LISTS, 4, "cpu", "t"), want)
    flat = np.asarray([v for l in LISTS for v in l], np.int64)
    off = np.concatenate([[0], np.cumsum([len(l) for l in LISTS])])
    for pair in ((off, flat), (off.tolist(), flat.tolist())):   # host pairs: arrays, plain lists
        for as_is in (True, False):
            _same(exclusions_on_device(pair, 4, "cpu", "t", as_is=as_is), want)


def test_a_pair_on_the_device_is_the_same_storage_or_sorted():
    off = torch.tensor([0, 3, 3, 7, 8], dtype=torch.int64)
    ids = torch.tensor([4, 2, 4, 9, 0, 7, 7, 3], dtype=torch.int32)      # neither ascending nor distinct: taken as it is
    o, i = exclusions_on_device((off, ids), 4, "cpu", "t")
    assert o.data_ptr() == off.data_ptr() and i.data_ptr() == ids.data_ptr() and o.tolist() == off.tolist() and i.tolist() == ids.tolist()
    o, i = exclusions_on_device((off, ids), 4, torch.device("cpu"), "t", as_is=False)
    assert i.data_ptr() != ids.data_ptr()
    _same((o, i), exclusion_csr(LISTS, 4))
    assert ids.tolist() == [4, 2, 4, 9, 0, 7, 7, 3]             # the caller's tensors are not written


def test_no_ids_give_the_one_element_dummy():
    for excl, as_is in (([[], [], []], True), ((np.zeros(4, np.int64), np.zeros(0, np.int32)), True),
                        ((torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)), True),
                        ((torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)), False)):
        off, ids = exclusions_on_device(excl, 3, "cpu", "t", as_is=as_is)
        assert off.tolist() == [0, 0, 0, 0] and ids.tolist() == [0] and ids.dtype == torch.int32


@pytest.mark.parametrize("what, dtype_error", CALLERS)
def test_what_each_caller_raises(what, dtype_error):
    kw = {"dtype_error": dtype_error} if dtype_error is not ValueError else {}
    off, ids = torch.tensor([0, 1, 2], dtype=torch.int64), torch.tensor([5, 6], dtype=torch.int32)
    for pair in ((off.to(torch.int32), ids), (off, ids.to(torch.int64))):
        with pytest.raises(dtype_error, match=r"%s: device exclusions are \(int64 offsets\[3\], int32 ids\)" % what):
            exclusions_on_device(pair, 2, "cpu", what, **kw)
    with pytest.raises(ValueError, match=r"%s: device exclusions .* n \+ 1 = 4 entries, got 3" % what):   # wrong offsets length
        exclusions_on_device((off, ids), 3, "cpu", what, **kw)
    with pytest.raises(ValueError, match="2 lists for 3 queries"):                                     # wrong number of lists
        exclusions_on_device([[1], [2]], 3, "cpu", what, **kw)
    with pytest.raises(ValueError, match="offsets must be non-decreasing from 0"):                     # a host pair: exclusion_csr's checks
        exclusions_on_device((np.asarray([0, 2, 1]), np.asarray([5])), 2, "cpu", what, **kw)
    with pytest.raises(ValueError, match="offsets must be non-decreasing from 0"):                     # ... a device pair too, not as is
        exclusions_on_device((off, ids), 3, "cpu", what, as_is=False, **kw)
    with pytest.raises(IndexError, match="does not fit int32"):
        exclusions_on_device([[2 ** 31], []], 2, "cpu", what, **kw)


def test_exclusion_lists_of_the_model_calls():
    users = ["7", "3", "9"]
    assert _exclusion_lists({"7": [1, 2], "9": (4,)}, users, "topk") == [[1, 2], (), (4,)]       # a missing key excludes nothing
    assert _exclusion_lists({}, users, "topk") == [(), (), ()]
    aligned = ([5], [], [6, 6])
    assert _exclusion_lists(aligned, users, "topk_head") == [[5], [], [6, 6]]
    assert _exclusion_lists(list(aligned), np.asarray([7, 3, 9]), "topk_head") == [[5], [], [6, 6]]
    for what in ("topk", "topk_head", "topk_markets_excluding"):
        with pytest.raises(ValueError, match="%s: 2 exclusion lists for 3 users" % what):
            _exclusion_lists([[1], [2]], users, what)
