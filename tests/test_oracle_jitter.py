"""Oracle.set_proj_view (CPU, no device): the oracle's forward prepass drawn with a matrix it is given -- the test infrastructure that holds
the HIP prepass under arctic_set_camera_jitter to the oracle's bytes (tests/test_gpu_jittered_prepass.py).  The hook is checked against what
it must not change (the camera's own matrix gives the unset bytes; the shadow map and the sky never see it) and against an independent
measure of what it must change (the float64 projection of every covered pixel's world position lies at the moved sample); and every case
of the GPU file is shown not to be vacuous, from the oracle alone."""
import numpy as np

import jitter_cases as J


def _frame(o, sc):
    return [x.copy() for x in J.planes(o)] + [o.read_shadow_map().view(np.uint32).copy() if sc.shadow_size else np.zeros(1, np.uint32),
                                              o.render_frame(sc.desc, sc.settings).copy(), o.stats().copy()]


def test_the_cameras_own_matrix_gives_the_unset_bytes(pkg, oracle):
    for sc in (pkg.scenes.config3(scale=0.1), pkg.scenes.config1(scale=0.5), J.ragged_cases(pkg)[1].sc):
        unset = J.oracle_prepass(oracle, sc)
        want = _frame(unset, sc)
        assert (want[1] != J.NO).sum() >= 38
        given = J.oracle_prepass(oracle, sc)
        given.set_proj_view(oracle.frame_constants(sc.desc)[0])
        given.pass_shadow_map(sc.desc); given.pass_gbuffer(sc.desc)
        for a, b in zip(want, _frame(given, sc)):
            assert a.tobytes() == b.tobytes(), sc.name
        given.set_proj_view(J.proj_view(oracle, sc.desc, sc.width, sc.height, J.CORNER_A))      # ... a jittered one does not ...
        given.pass_gbuffer(sc.desc)
        assert J.planes(given)[3].tobytes() != want[3].tobytes(), sc.name
        given.set_proj_view(None)                                                              # ... and NULL is the camera's again
        given.pass_shadow_map(sc.desc); given.pass_gbuffer(sc.desc)
        for a, b in zip(want, _frame(given, sc)):
            assert a.tobytes() == b.tobytes(), sc.name
        unset.close(); given.close()


def test_the_jittered_samples_lie_at_p_plus_half_minus_j(pkg, oracle):
    """the float64 projection of each covered pixel's world attribute through the UNJITTERED matrix lies at p + 0.5 - j.  The bound is four
    times the largest such distance of the unjittered oracle frame of the same scene (tests/test_gpu_taa.py's rule: the margin covers the
    two extra roundings per matrix row); both are printed"""
    scenes = [(pkg.scenes.config3(scale=0.1), J.JITTERS), (pkg.scenes.config1(scale=0.5), (J.EXISTING, J.CORNER_B, J.TINY)),
              (J.ragged_cases(pkg)[0].sc, J.RAGGED_JITTERS), (J.ragged_cases(pkg)[1].sc, J.RAGGED_JITTERS)]
    for sc, jitters in scenes:
        W, H = sc.width, sc.height
        o = J.oracle_prepass(oracle, sc, shadow=False)
        zero = J.planes(o)
        d0 = J.distance_to_sample(oracle, sc.desc, zero[0], zero[1], W, H, (0.0, 0.0)).max()
        o.close()
        for j in jitters:
            o = J.oracle_prepass(oracle, sc, j, shadow=False)
            p = J.planes(o)
            o.close()
            dj = J.distance_to_sample(oracle, sc.desc, p[0], p[1], W, H, j)
            stayed = J.distance_to_sample(oracle, sc.desc, p[0], p[1], W, H, (0.0, 0.0))
            print(f"{sc.name} {W}x{H} {J.jid(j)}: distance to the sample position {dj.max():.3e} px over {len(dj)} pixels; j = 0 {d0:.3e} px; bound {4 * d0:.3e}")
            assert len(dj) >= 38 and dj.max() <= 4 * d0, (sc.name, j, float(dj.max()), float(d0))
            assert stayed.min() >= np.hypot(*j) - 4 * d0, (sc.name, j, float(stayed.min()))      # the samples have moved by j, not stayed


def test_only_the_forward_prepass_reads_the_matrix(pkg, oracle):
    """the shadow map keeps its bytes; the sky ray and the shading's eye keep the camera: a pixel without geometry in both frames keeps its
    colour, and a G-buffer shaded under a set matrix gives the bytes it gives under none"""
    sc = pkg.scenes.config2(scale=0.25)
    sc.environment = pkg.scenes.synthetic_hdri(64, 32)
    a, b = J.oracle_prepass(oracle, sc), J.oracle_prepass(oracle, sc, J.CORNER_A)
    assert a.read_shadow_map().tobytes() == b.read_shadow_map().tobytes() and (a.read_shadow_map() < 1.0).any()
    fa, fb = a.render_frame(sc.desc, sc.settings), b.render_frame(sc.desc, sc.settings)
    sky = (J.planes(a)[1] == J.NO) & (J.planes(b)[1] == J.NO)
    assert sky.sum() >= 300 and (fa[sky][:, :3].sum(-1) > 0).all() and fa[sky].tobytes() == fb[sky].tobytes()
    assert fa.tobytes() != fb.tobytes()
    attrs, mat, _, _ = b.read_gbuffer()
    a.write_gbuffer(attrs, mat)                                                  # b's jittered G-buffer, shaded by an oracle that has no matrix set
    a.pass_shade(sc.desc, sc.settings); b.pass_shade(sc.desc, sc.settings)
    for x, y in zip(a.read_output(), b.read_output()):
        assert x.tobytes() == y.tobytes()
    a.close(); b.close()


def test_no_case_of_the_gpu_file_is_vacuous(pkg, oracle):
    """jitter_cases' conditions for every scene x jitter pair of tests/test_gpu_jittered_prepass.py, and the sweep's: every side of the frame
    has an offset at which the quad is drawn under one corner jitter and not under its opposite"""
    bad = []
    for case in J.all_cases(pkg, oracle):
        for j in case.jitters:
            n, differ, bits, ok = case.conditions(oracle, j)
            print(f"{case.id} {case.sc.width}x{case.sc.height} {J.jid(j)}: {n} covered pixels, {differ:.4f} of them differ from the unjittered frame, matrices differ: {bits}")
            if not ok:
                bad.append((case.id, J.jid(j), n, differ, bits))
    assert not bad, bad
    found = J.sweep_tells_the_matrices_apart(pkg, oracle)
    print("the sweep: offsets drawn under one corner jitter and not under its opposite:", found)
    import test_gpu_cluster_cull as CL
    assert all(found.get(side) for side in CL.SWEEP_SIDES), found
    for j in J.SWEEP_JITTERS:                                                    # the sweep's own counter: the quad is seen at 12 offsets or more
        assert sum(int((p[1] != J.NO).any()) for _, _, _, p, _ in J.oracle_sweep(pkg, oracle, j)) >= 12
        # ... and the number of clusters skipped tells the drawn matrix from the camera's at 8 offsets or more, on every side
        tells = [side for (side, _, _, _, _), (n, n0, safe) in zip(J.oracle_sweep(pkg, oracle, j), J.sweep_expected_skips(pkg, oracle, j)) if safe and n != n0]
        print(f"the sweep under {J.jid(j)}: the skipped clusters differ between the drawn and the camera's matrix at {len(tells)} offsets")
        assert len(tells) >= 8 and set(tells) == set(CL.SWEEP_SIDES), tells
