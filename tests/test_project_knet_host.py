"""Host-side checks (no GPU) of the fused projection + k-net entry: include/dgg_hip_next.h declares it in a block of its own, which parses
and binds from dgg_amd._lib.NEXT_BLOCKS["project_knet"] while NEXT_PROTOTYPES (the header's first block) stays what it was; the kernel
contract carries the new name with the parameters dgg_amd.ops takes."""
import ctypes
import inspect


ENTRY = "dgg_project_knet_fwd"


def test_the_block_parses_and_binds():
    import dgg_amd
    L_ = dgg_amd._lib
    assert set(L_.NEXT_BLOCKS["project_knet"]) == {ENTRY}
    restype, argtypes = L_.NEXT_BLOCKS["project_knet"][ENTRY]
    P, I = ctypes.c_void_p, ctypes.c_int
    #          x  N               d  nseg W  b  out lay act y  knet_seg deg mu_sd W1 b1 Wmu bmu Wp bp k  u  force stream
    assert argtypes == [P, ctypes.c_int64, I, I, P, P, P, P, P, P, I, P, P, P, P, P, P, P, P, P, P, I, P]
    assert restype is ctypes.c_int
    raw = ctypes.CDLL(L_.SO_PATH)
    assert hasattr(raw, ENTRY), f"libdgg_hip.so does not export {ENTRY}"
    fn = getattr(L_.bind(raw, [ENTRY]), ENTRY)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes
    assert list(getattr(L_.lib(), ENTRY).argtypes) == argtypes          # lib() binds every block


def test_the_first_block_and_the_recorded_abi_do_not_see_it():
    import dgg_amd
    L_ = dgg_amd._lib
    assert set(L_.NEXT_PROTOTYPES) == set(L_.NEXT_RESTYPES) == {"dgg_edgelist_topk_chunked", "dgg_edgelist_topk_p_chunked"}
    assert ENTRY not in L_.PROTOTYPES
    assert "project_knet" not in L_.NEXT_BLOCKS["norm_spmm"] and ENTRY not in L_.NEXT_BLOCKS["norm_spmm"]


def test_contract_and_ops_agree_on_the_new_entry():
    from dgg_amd import ops
    from dgg_amd.parallel import KernelContract
    params = [p for p in inspect.signature(KernelContract.project_knet).parameters if p != "self"]
    assert params == ["x", "layers", "knet_seg", "deg", "mu_sd", "W1", "b1", "Wmu", "bmu", "Wp", "bp"]
    assert list(inspect.signature(ops.project_knet).parameters)[:len(params)] == params
    assert KernelContract().project_knet(*[None] * len(params)) is None
    assert ops.PROJECT_KNET_FORCE is None
