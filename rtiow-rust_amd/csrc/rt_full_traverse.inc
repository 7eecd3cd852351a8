// rt_full_traverse.inc -- included INSIDE the traverse loop of the full-feature kernels: one box run or one slow pass over the
// including kernel's per-lane traversal state (op, o, d, inv, best, pc, cur_lo / cur_hi, the hit record ...), `tune`, `stack`;
// RT_R_PIXEL / RT_R_EVENT = the including kernel's expressions for the ray's pixel index and event number (its RNG stream);
// RT_FULL_SLOW_ARM = how it attaches the slow pass behind the box run: `else` or `if (!do_box)` (see there).
// RT_CENSUS (diagnostic builds, instrumented variant only): where the 64 lanes of the wave stand at every box step [0..15] and at
// every slow-pass iteration [16..31]: +0 BOX, +1 END (finished, waiting for a service), +2 no ray, +3 held at a gather point,
// +4.. = op (SPHERE 6, RECT 7, PUSH 8, POP 9, MEDIUM 10, PRISM 11, BEND 12), +15 = iterations
#if defined(RT_CENSUS) && defined(RT_CENSUS_HERE)  // (the pool kernel only)
#define RT_CENSUS_AT(base_) \
    if (COUNT) { \
      const uint32_t cop_ = have_ray ? (op == 0xfeu ? 0xfeu : (cur_hi.w & 0xffu)) : 0xffu; \
      const bool held_ = cop_ == 0xfeu || (RT_SLOW_OP(cop_) && (cur_hi.w & F_GATHER) != 0u && !release); \
      const uint32_t cls_ = !have_ray ? 2u : held_ ? 3u : cop_ == OP_BOX ? 0u : cop_ == OP_END ? 1u : 4u + (cop_ <= 8u ? cop_ : 8u); \
      _Pragma("unroll") for (uint32_t c_ = 0; c_ < 13u; c_++) { \
        const uint32_t n_ = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(cls_ == c_)); \
        if (lane == c_) census[(base_) / 16u] += n_; \
      } \
      if (lane == 15u) census[(base_) / 16u] += 1u; \
    }
#else
#define RT_CENSUS_AT(base_)
#endif
    const uint64_t b_box = __builtin_amdgcn_ballot_w64(op == OP_BOX);
    // Lanes at a gather point (head of a list-level run of records every ray executes in the same order)
    // are held until `gather_min` of them wait there -- or nothing else can run -- and then walk the run
    // together: one record kind per iteration, many lanes wide, instead of a few lanes per kind.
    const bool is_slow = RT_SLOW_OP(op);
    const bool at_gather = is_slow && (cur_hi.w & F_GATHER) != 0u;
    const uint64_t b_gather = __builtin_amdgcn_ballot_w64(at_gather);
#ifndef RT_GATHER_LOW
#define RT_GATHER_LOW 64  // (experiment) a slow pass that runs anyway -- no lane stands at a BOX record -- also releases a gather of this many lanes
#endif
    const bool release = (uint32_t)__builtin_popcountll(b_gather) >= tune.gather_min ||
                         (b_box == 0 && ((uint32_t)__builtin_popcountll(b_gather) >= RT_GATHER_LOW ||
                                         __builtin_amdgcn_ballot_w64(is_slow && !at_gather) == 0));
    const bool runnable = is_slow && (!at_gather || release);
    const uint64_t b_slow = __builtin_amdgcn_ballot_w64(runnable);
    // The two arms on one wave-uniform flag.  RT_FULL_SLOW_ARM (the including kernel's) is how the slow pass is attached:
    // `else`, or `if (!do_box)` -- the same arm in every state, but the second form leaves the compiler no join of two arms at
    // which to keep a second copy of the walk's registers (rt_pool.h, traverse loop).  Which form a kernel takes is decided on
    // its ISA (profiles/r15_traverse_shape/README.txt): the lock-step kernel loses 52 VALU and up to 23 VGPRs with the second,
    // the first pool kernel's LIST / GENB instantiations gain spills with it.
    const bool do_box = b_box != 0 && (uint32_t)__builtin_popcountll(b_slow) < tune.sphere_min;
    if (do_box) {
#ifdef RT_PHASE_PRIO
      __builtin_amdgcn_s_setprio(RT_FULL_BOX_PRIO);
#endif
      const uint32_t n0 = (uint32_t)__builtin_popcountll(b_box);
      const uint32_t floor_lanes = n0 > tune.box_leave ? n0 - tune.box_leave : 0u;
      uint32_t n_now;
      if (COUNT) t_mark = RT_TICK();
      do {
        if (COUNT) n_box_it++;
        RT_CENSUS_AT(0u);
#define RT_FULL_BOX_STEP() \
        if (op == OP_BOX) {  /* Aabb::hit, aabb.rs:16-27 (1/d and its sign re-read: d changes under RotateY/Scale) */ \
          if (COUNT) cnt.aabb++; \
          if (hi_is_root(cur_hi)) root_hits = nhits;  /* (never set inside a boundary stream: the flattener leaves those roots unmarked) */ \
          /* plain f32 math: packed v_pk_* instructions are slower than the pairs they replace on gfx950 (rt_pool.h RT_PK_MATH) */ \
          f32x2 tx, ty, tz; \
          tx.x = (u2f(cur_lo.x) - o.x) * inv.x, tx.y = (u2f(cur_lo.y) - o.x) * inv.x; \
          ty.x = (u2f(cur_lo.z) - o.y) * inv.y, ty.y = (u2f(cur_lo.w) - o.y) * inv.y; \
          tz.x = (u2f(cur_hi.x) - o.z) * inv.z, tz.y = (u2f(cur_hi.y) - o.z) * inv.z; \
          float ax = inv.x < 0.f ? tx.y : tx.x, bx = inv.x < 0.f ? tx.x : tx.y; \
          float ay = inv.y < 0.f ? ty.y : ty.x, by = inv.y < 0.f ? ty.x : ty.y; \
          float az = inv.z < 0.f ? tz.y : tz.x, bz = inv.z < 0.f ? tz.x : tz.y; \
          float start = rs_max(GENB ? t_lo : t_near, rs_max(rs_max(ax, ay), az)); \
          float end = rs_min(best, rs_min(rs_min(bx, by), bz)); \
          RT_FULL_BOX_ADVANCE(end > start); \
          op = cur_hi.w & 0xffu; \
          RT_FULL_FAT_LEAF(); \
        }
// RT_FAT_LEAF: a lane whose box step lands on a plain SPHERE record (the object of a Bvh leaf whose box it has just passed)
// executes it in the same step instead of parking: inside a Bvh of spheres lanes then never leave the box loop
#if RT_FAT_LEAF
#define RT_FULL_FAT_LEAF() \
          if (op == OP_SPHERE && (cur_hi.w & (F_MOVE | F_GATHER)) == 0u) { \
            exec_op(OP_SPHERE, o, d, inv, time, best, pc, cur_lo, cur_hi, hp, hn, hmat, depth, tag, nhits, root_hits, ev_draws, RT_R_PIXEL, r_sample, \
                    RT_R_EVENT, stack, sv_o, sv_d, bmode, t_lo, b_saved, b_t1); \
            cur_lo = RT_FETCH_LO(pc), cur_hi = RT_FETCH_HI(pc), op = cur_hi.w & 0xffu; \
          }
#else
#define RT_FULL_FAT_LEAF()
#endif
#define RT_FULL_BOX_ADVANCE(pass_) \
          pc = (pass_) ? pc + RSZ : cur_hi.z; \
          cur_lo = RT_FETCH_LO(pc), cur_hi = RT_FETCH_HI(pc)
        RT_FULL_BOX_STEP();
#if RT_FULL_BOX_UNROLL >= 2
        RT_FULL_BOX_STEP();  // lanes that left the BOX state sit this one out; the schedule check runs every other step
#endif
#undef RT_FULL_BOX_STEP
#undef RT_FULL_BOX_ADVANCE
#undef RT_FULL_FAT_LEAF
        n_now = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(op == OP_BOX));
        if (COUNT) n_box_lanes += n_now;
      } while (n_now > floor_lanes);
      if (COUNT) t_box += RT_TICK() - t_mark;
    }
    RT_FULL_SLOW_ARM {
      // ---- slow pass: every parked lane executes one record, then runs ahead through up to
      // `run_ahead` - 1 more while enough lanes still sit on slow records (the objects of a list world
      // are visited in the same order by every ray, so these lanes mostly share their next kinds) ----
      if (COUNT) t_mark = RT_TICK();
#ifdef RT_PHASE_PRIO
      __builtin_amdgcn_s_setprio(RT_FULL_SLOW_PRIO);
#endif
      if (!runnable) op = 0xfeu;  // held at a gather point: sits this pass out
      // (one iteration at least, also when no lane is runnable -- which only happens when the including loop is about to leave:
      // a guarded loop made the compiler copy 33 loop-carried registers once more in front of the guard)
      bool more;
      uint32_t ahead = 0;
#pragma unroll 1
      do {
      RT_CENSUS_AT(16u);
      if (COUNT) n_slow_it++, n_slow_lanes += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(RT_SLOW_OP(op)));
      exec_op(op, o, d, inv, time, best, pc, cur_lo, cur_hi, hp, hn, hmat, depth, tag, nhits, root_hits, ev_draws, RT_R_PIXEL, r_sample,
              RT_R_EVENT, stack, sv_o, sv_d, bmode, t_lo, b_saved, b_t1);
      if (RT_SLOW_OP(op)) {
        cur_lo = RT_FETCH_LO(pc), cur_hi = RT_FETCH_HI(pc), op = cur_hi.w & 0xffu;
        if ((cur_hi.w & F_GATHER) && !release) op = 0xfeu;  // arrived at a gather point: wait for the next batch
      }
      ahead++;
      {  // run ahead while enough lanes sit on slow records -- or while NO lane waits at a BOX record: then nobody is held up, and a
         // thin wave (the drain at the end of a launch: a handful of long paths) walks a list-level run in one pass, not one pass per record
        const uint64_t m_sl = __builtin_amdgcn_ballot_w64(RT_SLOW_OP(op));
        more = ahead < tune.run_ahead && ((uint32_t)__builtin_popcountll(m_sl) >= tune.run_ahead_min ||
                                          (RT_RUN_AHEAD_NOBOX && m_sl != 0 && __builtin_amdgcn_ballot_w64(op == OP_BOX) == 0));
      }
      } while (more);
      if (COUNT) t_slow += RT_TICK() - t_mark;
    }
#undef RT_CENSUS_AT
