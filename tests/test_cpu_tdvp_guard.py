"""CPU tests of the operand check in front of every device-pointer call of the TDVP path (tdvp._operands): the kernels read raw memory
with one element type, so an operand of another dtype (a real environment next to a complex site: read as interleaved complex, past
its end), a strided or lazily conjugated view, or a host tensor must raise TTNError before the library is called.  Every wrapper runs
the check first, so CPU tensors reach it and nothing touches a device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def D():
    import ttn_amd
    return ttn_amd.tdvp


def _t(shape, dtype):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    return x.to(dtype) if dtype != torch.complex128 else torch.complex(x, x.flip(0))


def test_operands_accepts_one_dtype_and_names_the_flag(D):
    # (CPU tensors pass the dtype and layout checks and stop at the device check, which comes last)
    for dt in (torch.float64, torch.complex128):
        with pytest.raises(D._lib.TTNError, match="not all on the GPU"):
            D._operands(_t((3, 2, 3), dt), _t((3, 2, 3), dt))


@pytest.mark.parametrize("dts", [(torch.float64, torch.complex128), (torch.complex128, torch.float64, torch.complex128),
                                 (torch.float32,), (torch.complex64, torch.complex64), (torch.float64, torch.float32)])
def test_operands_rejects_dtypes(D, dts):
    with pytest.raises(D._lib.TTNError, match="one dtype, float64 or complex128"):
        D._operands(*[_t((2, 3, 2), dt) for dt in dts])


def test_operands_rejects_views(D):
    a = _t((4, 2, 4), torch.float64)
    with pytest.raises(D._lib.TTNError, match="view"):
        D._operands(a, a.transpose(0, 2))
    c = _t((4, 2, 4), torch.complex128)
    assert c.conj().is_conj()
    with pytest.raises(D._lib.TTNError, match="view"):
        D._operands(c, c.conj())


def test_every_wrapper_checks_before_the_library(D):
    """The mixed-dtype launch of a real-input sweep: real F and M next to a complex AC.  Each device-pointer wrapper raises TTNError
    from the check (a host tensor would otherwise reach the device lookup, which raises a different message without a GPU)."""
    r, c = torch.float64, torch.complex128
    Dl, d, Dr, a = 3, 2, 4, 2
    AC, FL, FR, M = _t((Dr, d, Dl), c), _t((Dl, a, Dl), r), _t((Dr, a, Dr), r), _t((d, a, d, a), r)
    calls = [
        lambda: D._d_applyH1(AC, FL, FR, M),
        lambda: D._d_applyH0(_t((Dr, Dl), c), FL, FR),
        lambda: D._d_left_env(AC, M, FL),
        lambda: D._d_right_env(AC, M, FR),
        lambda: D._d_applyH2(_t((Dr, d, d, Dl), c), FL, FR, M, M),
        lambda: D._qr_j(_t((Dr, d * Dl), torch.float32)),
        lambda: D._svd_j(_t((Dr, d * Dl), torch.complex64)),
    ]
    for call in calls:
        with pytest.raises(D._lib.TTNError, match="one dtype"):
            call()


def test_real_parts_rule(D):
    """the store of a complex result into a real ψ: real parts when the imaginary parts vanish, InexactError as TTNError otherwise"""
    x = np.arange(6.0).reshape(1, 2, 3)
    out = D._real_parts([x + 0j, x + 1e-14j], "ψ")
    assert all(o.dtype == np.float64 and np.array_equal(o, x) for o in out)
    with pytest.raises(D._lib.TTNError, match="InexactError"):
        D._real_parts([x + 0j, x + 1e-9j], "ψ")
