"""dgg_amd.parallel.KernelContract -- what ShardedDGGConv may call beyond the baseline entries -- against the two kernel namespaces there
are: dgg_amd.ops provides every name with parameters the contract's calls bind to, and the numpy stand-in of the host tests leaves every
optional entry at the contract's "absent" answer.  No GPU, no compiled library (dgg_amd.ops loads it on first use)."""
import inspect

from dgg_amd import ops
from dgg_amd.parallel import KernelContract, ShardedDGGConv
from test_parallel_gloo import CpuKern
from test_sharded_edgelist_host import RowKern

NAMES = [n for n in vars(KernelContract) if not n.startswith("_")]
FLAGS = [n for n in NAMES if not callable(vars(KernelContract)[n])]
ENTRIES = [n for n in NAMES if callable(vars(KernelContract)[n])]


def test_ops_provides_every_name_of_the_contract():
    assert sorted(FLAGS) == ["DA_MAP", "EMLP_BWD_PARTP", "KNET_MFMA_WIDTHS", "PREMASK"] and len(ENTRIES) > 15
    for n in FLAGS:
        assert type(getattr(ops, n)) is type(getattr(KernelContract, n)), n
        assert not getattr(KernelContract, n), f"{n}: the contract's flags are off"
    for n in ENTRIES:
        params = [p for p in inspect.signature(getattr(KernelContract, n)).parameters if p != "self"]
        inspect.signature(getattr(ops, n)).bind(**dict.fromkeys(params))        # raises TypeError on a name ops does not take
        # (the engine passes leading arguments by position: the same order as ops, from the first parameter on)
        assert list(inspect.signature(getattr(ops, n)).parameters)[:len(params)] == params, n


def test_stand_in_leaves_every_optional_entry_absent():
    for kern in (CpuKern(), RowKern()):
        lay = ShardedDGGConv(kern, 8)
        kern = lay.kern
        assert lay._rsym_status is False, "the stand-in's allpairs_topk takes no status="
        for n in FLAGS:
            assert getattr(kern, n) is getattr(KernelContract, n), n
        for n in ENTRIES:
            fn = getattr(kern, n)
            assert fn.__func__ is vars(KernelContract)[n], f"{n}: the stand-in shadows the contract's default"
            nargs = sum(p.default is p.empty for p in inspect.signature(fn).parameters.values())
            assert fn(*([None] * nargs)) is None, n
    lay = ShardedDGGConv(ops, 8)
    assert lay.kern is ops and lay._rsym_status is True


def test_object_namespace_that_does_not_inherit_gets_the_contract_behind_it():
    """an object with baseline entries only (the stand-in of this suite's earlier version) keeps working: the contract becomes a base
    of its class; a MODULE is never touched, so a name dgg_amd.ops lacked would raise AttributeError where it is called"""
    class Plain:
        def linear_fwd(self, x, W, b, act, w_layout):
            return "own"

    plain = Plain()
    lay = ShardedDGGConv(plain, 8)
    assert lay.kern is plain and isinstance(plain, KernelContract) and type(plain).__name__ == "Plain"
    assert plain.linear_fwd(0, 0, 0, 0, 0) == "own" and plain.partp_sort(None) is None and lay._rsym_status is False
    assert not isinstance(ShardedDGGConv(ops, 8).kern, KernelContract)
