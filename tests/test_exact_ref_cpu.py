"""Pins tests/_exact_ref.py without a GPU: for every operand class at every shape tests/test_hip_conv_exact.py uses, the
class condition mag / unit <= 2^22 holds for every output element and the float64 reference is unchanged by a round trip
through f32 (both asserted by the generators themselves: building a case is the check); a plain restatement of
conv_pw_h2_kernel's arithmetic - the scale per 32-row block (and per wave: 64 rows on the 128-row tiles) from the first
non-zero K-tile, the scaled activations as two f16 planes, pack_h2's own split of the weights, the three kept products summed
in float64, the scales out again - returns the reference EXACTLY, and so do the six kept terms of the x3 split; the weight lo
plane (x3: the third plane of both operands) of the packed image is all zero - but for two_plane_w, whose activation lo plane is.  The restatements are the reference's witness
that a mismatch on the GPU is the kernel's and not the class's."""
import pytest
import torch

import _exact_ref as R

_H2 = sorted({(rows, K, N, 2 if bm == 1064 else 1) for bm, rows, N, K in R.H2_GEMM})


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('cls', R.CLASSES)
@pytest.mark.parametrize('rows,K,N,kgroups', _H2)
def test_h2_restatement_returns_the_reference(rows, K, N, kgroups, cls, scaled):
    from fgn_amd import ops
    c = R.gemm_case(rows, K, N, cls, 'h2', scaled, kgroups)
    hi, lo, inv = R.unpack_h2(ops.pack_h2(c['w'][0]), 1, N, K)
    S = R.h2_scales(c['x'][0].double(), 32, kgroups).repeat_interleave(32, 1)
    xs = (c['x'][0].double() * S).float()
    a_lo = (xs != xs.half().float()).any()                   # the activation lo plane is in use
    if cls == 'two_plane_w':                                 # weights of up to 22 bits against activations of up to 11
        assert (lo != 0).any() and not a_lo
    else:
        assert (lo == 0).all()                               # at most 11 significant bits: h alone holds a weight
        assert torch.equal(hi[0, :N] * inv[0, :N, None], c['w'][0].double())
        assert a_lo == (cls in ('two_plane', 'rows_apart15'))
    assert torch.equal((hi[0, :N] + lo[0, :N]) * inv[0, :N, None], c['w'][0].double())
    for block in ((32, 64) if kgroups == 1 else (32,)):
        got = R.h2_restate(c['x'][0], hi[0], lo[0], inv[0], N, block, kgroups)
        assert torch.equal(got, c['prod'][0]), (block, int((got != c['prod'][0]).sum()))


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('cls', R.CLASSES)
@pytest.mark.parametrize('bm,groups,grp_rows,valid,K,N', R.H2_GROUPED)
def test_grouped_h2_restatement(bm, groups, grp_rows, valid, K, N, cls, scaled):
    from fgn_amd import ops
    c = R.gemm_case(valid, K, N, cls, 'h2', scaled, groups=groups)
    hi, lo, inv = R.unpack_h2(ops.pack_h2(c['w']), groups, N, K)
    assert (lo != 0).any() if cls == 'two_plane_w' else (lo == 0).all()
    for gi in range(groups):
        got = R.h2_restate(c['x'][gi], hi[gi], lo[gi], inv[gi], N, R.h2_block(bm))
        assert torch.equal(got, c['prod'][gi])


def test_k_steps_moves_the_scale_as_the_class_says():
    """One K-group, five K-tiles: a new scale at the tile 2^3 above, none at the one 2^2 above that nor at the one 2^10 below
    (a scale only ever moves to make room); blocks whose first K-tile is zero take theirs from the second."""
    c = R.gemm_case(130, 160, 260, 'k_steps', 'h2')
    S = R.h2_scales(c['x'][0].double(), 32)[::32]          # [blocks, K-tiles]
    assert (S[0, 1] == S[0, 0] / 8).all() and (S[0, 2] == S[0, 1]).all() and (S[0, 3] == S[0, 2]).all()
    assert (c['x'][0][32:64, :32] == 0).all() and S[1, 1] == S[0, 1]
    two = R.h2_scales(R.gemm_case(2111, 320, 1024, 'k_steps', 'h2', kgroups=2)['x'][0].double(), 32, 2)[0]
    assert two[2] == two[0] / 8 and two[4] == two[2] and two[3] == two[1]      # each K-group follows its own tiles


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('cls', R.X3_CLASSES)
@pytest.mark.parametrize('groups,grp_rows,valid,K,N', R.X3_GEMM)
def test_x3_restatement_returns_the_reference(groups, grp_rows, valid, K, N, cls, scaled):
    from fgn_amd import ops
    c = R.gemm_case(valid, K, N, cls, 'x3', scaled, groups=groups)
    planes = R.unpack_x3(ops.pack_x3(c['w']), groups, N, K)
    assert (planes[2] == 0).all()                          # at most 16 significant bits: the dropped terms vanish
    for gi in range(groups if groups < 4 else 2):
        assert (R.x3_planes(c['x'][gi])[2] == 0).all()
        got = R.x3_restate(c['x'][gi], [p[gi] for p in planes], N)
        assert torch.equal(got, c['prod'][gi])
    if cls == 'two_plane':
        assert (planes[1] != 0).any() and (R.x3_planes(c['x'][0])[1] != 0).any()


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('name', sorted(R.conv_specs()))
def test_convolution_cases_meet_the_condition(name, scaled):
    for cls in R.conv_specs()[name][1]:
        c = R.conv_case(cls=cls, scaled=scaled, **R.conv_specs()[name][0])
        assert all(torch.isfinite(r).all() for r in c['refs'])


@pytest.mark.parametrize('rows,cin1,cin2,cout,arith', R.DUAL)
def test_dual_and_gradient_cases_meet_the_condition(rows, cin1, cin2, cout, arith):
    for cls in R.CLASSES:
        for scaled in (False, True):
            c = R.dual_case(rows, cin1, cin2, cout, arith, cls, scaled)
            folded = torch.cat((c['w1'].view(cout, cin1).double() * (c['bn1']['weight'] / torch.sqrt(c['bn1']['running_var'] + 1e-5))[:, None],
                                c['w2'].view(cout, cin2).double() * (c['bn2']['weight'] / torch.sqrt(c['bn2']['running_var'] + 1e-5))[:, None]), 1)
            assert torch.equal(folded, c['w'][0].double())
    for shape in R.TN_GEMM:
        R.grad_case(*shape)
    for m, k, n, _, _ in R.SMALL_GEMM:
        R.grad_case(k, m, n)


def test_the_condition_refuses_what_is_outside_the_class():
    """mag / unit above 2^22 is an assertion error in the generator, not a looser test"""
    mag, unit = torch.full((2, 2), 2.0 ** 22 + 1, dtype=torch.float64), torch.ones(2, 2, dtype=torch.float64)
    with pytest.raises(AssertionError):
        R.check_class(mag, unit)
    R.check_class(mag - 1, unit)
