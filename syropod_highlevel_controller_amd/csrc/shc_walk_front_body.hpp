// The front of WalkController::updateWalk (:440-527) that is the same for every leg of a robot - getLimit x 4 and the desired body velocities of this cycle - as
// a run of STATEMENTS, included (not called) where it runs: in cycle_front, and in walk_velocity_front (shc_cycle.hpp) for a wavefront that runs the front for
// another.  One text, so the two cannot drift apart; included, because the same statements behind a call - even a forced-inline one - reach the optimiser in
// another order and every cycle kernel comes out with other contractions and waits (measured: config 3 0.8 % slower).  No include guard: this is no header.
// Names the including scope provides: C, P, rb, g, fb, L, R; vin_x, vin_y, win (the command), walk_state (BEFORE this cycle's state machine), frozen; the
// outputs vx, vy, vw (declared by the includer; read from VLIN / VANG, rewritten), and it declares lin_norm (|linear input| or its stand-in).  Macros:
// SHC_FRONT_TIP_X / _Y (this leg's tip as the previous cycle left it), SHC_FRONT_WRITTEN_OUT (bool: contractions as explicit fmas, see bearing_bracket).
  // ---- getLimit x 4 (:414-436): bracket index per leg, min over the robot's legs
  double lim[4] = {0.05, 0.3, 0.02, 0.1};
  if (!(SHC_DBG(P) & 2)) {
    double sx = vin_x + win * (-SHC_FRONT_TIP_Y), sy = vin_y + win * SHC_FRONT_TIP_X;
    int idx = bearing_bracket<SHC_FRONT_WRITTEN_OUT>(sy, sx);
    if (__all(idx == fb.limit_bracket)) { // every leg of every robot of the wave in the bracket it was in: the same minima
#pragma unroll
      for (int k = 0; k < 4; ++k) lim[k] = fb.limit_value[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) lim[k] = kUnassigned;
#pragma unroll
      for (int j = 0; j < L; ++j) {
        int ij = g.get(idx, j);
#pragma unroll
        for (int k = 0; k < 4; ++k) lim[k] = fmin(lim[k], C.limit[ij][k]);
      }
      fb.limit_bracket = idx;
#pragma unroll
      for (int k = 0; k < 4; ++k) fb.limit_value[k] = lim[k];
    }
  }
  SHC_PHASE_FENCE();
  SHC_TICK(5);
  vx = rb.get(R::VLIN), vy = rb.get(R::VLIN + 1), vw = rb.get(R::VANG);
  // |linear input|.  Throttle mode only ever asks "> 1" and "!= 0" of it: while no robot of the wave has n2 > 1 (sqrt(n2) <= 1 then, the
  // correctly rounded square root being monotone with sqrt(1) = 1) a stand-in with the same two answers saves the FP64 square root.
  // (SHC_FRONT_WRITTEN_OUT, as in bearing_bracket: left to the compiler, which of the two squares is rounded depends on where the inputs come from - registers
  //  loaded from the tile in cycle_front, a shuffle on a wavefront that takes a fresh command itself.  The explicit form is the one the compiler picks in cycle_front.)
  double lin_n2;
  if constexpr (SHC_FRONT_WRITTEN_OUT) lin_n2 = fma(vin_x, vin_x, vin_y * vin_y);
  else lin_n2 = vin_x * vin_x + vin_y * vin_y;
  double lin_norm;
  const int velocity_input_mode = fb.uf.velocity_input_mode;
  if (velocity_input_mode == 0 && __all(lin_n2 <= 1.0)) lin_norm = lin_n2 != 0.0 ? 0.5 : 0.0;
  else lin_norm = sqrt(lin_n2);
  if (!(SHC_DBG(P) & 32)) {
    double nvx, nvy, nw;
    if (velocity_input_mode == 0) { // throttle (:451-466)
      double k = 1.0; // clamped to the unit disc
      if (__any(lin_norm > 1.0)) k = lin_norm > 1.0 ? 1.0 / lin_norm : 1.0;
      const double cx = lin_norm > 1.0 ? vin_x * k : vin_x, cy = lin_norm > 1.0 ? vin_y * k : vin_y;
      nw = clampd(win, -1.0, 1.0) * lim[1];
      const double sc = 1.0 - fabs(win);
      nvx = (cx * lim[0]) * sc;
      nvy = (cy * lim[0]) * sc;
    } else { // real (:467-481)
      const bool over = lin_norm > lim[0];
      const double k = lim[0] / lin_norm;
      const double cx = over ? vin_x * k : vin_x, cy = over ? vin_y * k : vin_y;
      nw = clampd(win, -lim[1], lim[1]);
      const double sc = lim[1] != 0.0 ? (1.0 - fabs(nw / lim[1])) : 0.0;
      nvx = cx * sc;
      nvy = cy * sc;
    }
    if (walk_state == WS_STOPPING) nvx = nvy = nw = 0.0; // :483-487
    if (frozen) nvx = vx, nvy = vy, nw = vw; // (a robot with a manual leg keeps its desired velocities: zero acceleration below)
    // acceleration-limited approach (:508-527)
    const double ax = nvx - vx, ay = nvy - vy;
    const double an2 = ax * ax + ay * ay;
    const double an = __all(an2 == 0.0) ? 0.0 : sqrt(an2); // (every robot already at its target velocity: sqrt(0) = 0)
    const double cap = lim[2] * P.dt;
    if (__all(an < cap)) { // every robot of the wave reaches its target this cycle (the steady state)
      vx += ax;
      vy += ay;
    } else {
      const double inv = an2 > 0.0 ? an : 1.0; // normalized() leaves the zero vector unchanged
      const double sx_ = (ax / inv) * lim[2] * P.dt, sy_ = (ay / inv) * lim[2] * P.dt;
      vx += an < cap ? ax : sx_;
      vy += an < cap ? ay : sy_;
    }
    const double aa = nw - vw;
    vw += fabs(aa) < lim[3] * P.dt ? aa : signd(aa) * lim[3] * P.dt;
    rb.put(R::VLIN, vx);
    rb.put(R::VLIN + 1, vy);
    rb.put(R::VANG, vw);
  }
