// rt_full_ops.inc -- included INSIDE the full-feature kernels (rt_pool_full.h, rt_sync_full.h): the per-record operations of
// the flat program as lambdas over the including kernel's locals (t_near, lc, sc, cnt, total_draws, lane, the RT_FETCH_* macros,
// the COUNT / GENB template parameters).  One text, two schedules.  RT_REG_STACK0 (defined by the includer) = 1: level 0 of the
// transform stack lives in the registers sv_o / sv_d instead of the per-wave scratch.
// RT_DEFER_HIT (defined by the includer) = 1: a hit is kept as (best, record pc | prism face | "textured" bit 3) in `hmat` -- no
// point, no normal, nothing for a POP to transform; the shade pass rebuilds the record from the ray and t, replaying the wrappers
// around the winning record (rt_pool_full.h rebuild_hit).  0: the hit record (hp, hn, material) rides in registers.
// SURF (the includer's template parameter): attribute triangles (FEAT_SURFACE).  Under RT_DEFER_HIT only the record step differs;
// without it the TRI case also writes the includer's h_tu / h_tv.  No other record resets them: only a material with MAT_SURFACE
// reads them, and the builder accepts such a material on triangles with UVs alone, which write them when they win.
  // ConstantMedium::hit once both boundary queries hit at t1, t2 (object.rs:553-574): clamp to the range, one draw from the
  // event's stream, exponential free path.  `med_lo / med_hi` = the MEDIUM record (density, material, flags).
  auto medium_between = [&](float t1, float t2, const uint4 med_lo, const uint4 med_hi, [[maybe_unused]] const uint32_t med_pc, const V3 o, const V3 d, float& best, V3& hp,
                            V3& hn, uint32_t& hmat, const uint32_t depth, uint32_t& tag, uint32_t& nhits, const uint32_t root_hits,
                            uint32_t& ev_draws, const uint32_t r_pixel, const uint32_t r_sample, const uint32_t r_event) {
    t1 = rs_max(t1, t_near);
    t2 = rs_min(t2, best);
    if (!(t1 >= t2)) {
      const uint64_t seed = ((uint64_t)load_const(&lc->P.seed_hi) << 32) | load_const(&lc->P.seed_lo);
      const float len = vlen(d);
      float distance_inside = (t2 - t1) * len;
      float hit_distance = -(1.f / u2f(med_lo.x)) * rt_logf(event_draw_f32(seed, r_pixel, r_sample, r_event, ev_draws));
      ev_draws++;
      if (COUNT) total_draws++;
      if (hit_distance < distance_inside) {
        float t = t1 + hit_distance / len;
        bool accept = !(med_hi.w & F_UNDER_BVH) || nhits == root_hits || !(best < t);
        if (accept) {
#if RT_DEFER_HIT
          hmat = med_pc | ((med_hi.w >> 16) & 8u);
          best = t, nhits++;
#else
          hp = vadd(o, smul(t, d)), hn = mk(1.f, 0.f, 0.f), hmat = med_hi.z | ((med_hi.w & F_TEXTURED) << 12);
          best = t, tag = depth, nhits++;
#endif
        }
      }
    }
  };

  // One non-BOX record for one ray.  The ray's registers are passed explicitly: the traversal lanes run
  // it on their own ray, the list pass on rays it loads from path slots.
  auto exec_op = [&](const uint32_t op, V3& o, V3& d, V3& inv, const float time, float& best, uint32_t& pc, const uint4 cur_lo,
                     const uint4 cur_hi, V3& hp, V3& hn, uint32_t& hmat, uint32_t& depth, uint32_t& tag, uint32_t& nhits,
                     const uint32_t root_hits, uint32_t& ev_draws, const uint32_t r_pixel, const uint32_t r_sample,
                     const uint32_t r_event, float* stack, V3& sv_o, V3& sv_d, uint32_t& bmode, float& t_lo, float& b_saved,
                     float& b_t1) {
    if (op == OP_SPHERE) {  // Sphere::hit, object.rs:84-111 (+ fused Translate / FlipNormals)
      // A lane that finds ANOTHER plain SPHERE record behind this one executes it right away (and so on): the spheres of a
      // list world stand in a row (main.rs:234-252), the lanes walk them together, and every record saved this way saves
      // one trip through the pass loop (kind dispatch, schedule ballots, the caller's fetch).  Same records, same order.
      uint4 s_lo = cur_lo, s_hi = cur_hi;
      for (;;) {
        if (COUNT) cnt.prim++;
        [[maybe_unused]] const uint32_t self_pc = pc;
        const V3 off = mk(u2f(s_lo.x), u2f(s_lo.y), u2f(s_lo.z));
        V3 lo_o = o;
        if (s_hi.w & F_TRANSLATE) lo_o = vsub(o, off);
        if (s_hi.w & F_MOVE) {  // LinearMove inside the Translate (object.rs:505-508): motion = the data record behind this one
          const uint4 mv = RT_FETCH_LO(pc + RSZ);
          lo_o = vsub(lo_o, smul(time, mk(u2f(mv.x), u2f(mv.y), u2f(mv.z))));
          pc += RSZ;
        }
        float t;
        if (sphere_hit_t(lo_o, d, u2f(s_lo.w), GENB ? t_lo : t_near, best, t)) {
          if (GENB && bmode) {
            best = t;  // boundary query: only the closest t matters
          } else {
#if RT_DEFER_HIT
            hmat = self_pc | ((s_hi.w >> 16) & 8u);
            best = t, nhits++;
#else
            V3 p = vadd(lo_o, smul(t, d));
            V3 n = sdiv(p, u2f(s_lo.w));
            if (s_hi.w & F_TRANSLATE) p = vadd(p, off);
            if (s_hi.w & F_FLIP) n = vneg(n);
            hp = p, hn = n, hmat = s_hi.z | ((s_hi.w & F_TEXTURED) << 12);
            best = t, tag = depth, nhits++;
#endif
          }
        }
        pc += RSZ;
        if (!RT_SAME_KIND_RUN) break;
        const uint4 n_hi = RT_FETCH_HI(pc);
        if ((n_hi.w & (0xffu | F_GATHER)) != (uint32_t)OP_SPHERE) break;
        s_lo = RT_FETCH_LO(pc), s_hi = n_hi;
      }
    } else if (op == OP_RECT) {  // Rect::hit, object.rs:185-218 (consecutive RECT records in one go: see OP_SPHERE)
      uint4 s_lo = cur_lo, s_hi = cur_hi;
      for (;;) {
        if (COUNT) cnt.prim++;
        const uint32_t axis = (s_hi.w >> F_AXIS_SHIFT) & 3u;
        float t;
        if (rect_hit_t(o, d, axis, u2f(s_lo.x), u2f(s_lo.y), u2f(s_lo.z), u2f(s_lo.w), u2f(s_hi.x), GENB ? t_lo : t_near, best, t)) {
          if (GENB && bmode) {
            best = t;
          } else {
#if RT_DEFER_HIT
            hmat = pc | ((s_hi.w >> 16) & 8u);
            best = t, nhits++;
#else
            V3 n = mk(axis == 0 ? 1.f : 0.f, axis == 1 ? 1.f : 0.f, axis == 2 ? 1.f : 0.f);
            if (s_hi.w & F_FLIP) n = vneg(n);
            hp = vadd(o, smul(t, d)), hn = n, hmat = s_hi.z | ((s_hi.w & F_TEXTURED) << 12);
            best = t, tag = depth, nhits++;
#endif
          }
        }
        pc += RSZ;
        if (!RT_SAME_KIND_RUN) break;
        const uint4 n_hi = RT_FETCH_HI(pc);
        if ((n_hi.w & (0xffu | F_GATHER)) != (uint32_t)OP_RECT) break;
        s_lo = RT_FETCH_LO(pc), s_hi = n_hi;
      }
    } else if (op == OP_PRISM) {  // rect_prism: six Rect::hit in one instruction
      if (COUNT) cnt.prim += 6;
      float t;
      uint32_t face = 0;
      const uint32_t nh = prism_hit_t(cur_lo, cur_hi, o, d, GENB ? t_lo : t_near, best, t, face);
      if (nh) {
        if (GENB && bmode) {
          best = t;
        } else {
#if RT_DEFER_HIT
          hmat = pc | face | ((cur_hi.w >> 16) & 8u);
          best = t, nhits += nh;
#else
          hp = vadd(o, smul(t, d)), hn = prism_normal(face), hmat = cur_hi.z | ((cur_hi.w & F_TEXTURED) << 12);
          best = t, tag = depth, nhits += nh;
#endif
        }
      }
      pc += RSZ;
    } else if (TRI && op == OP_TRI) {  // a triangle (flat_scene.h OP_TRI; rt_triangle.h): the TRI record and its data record
      if (COUNT) cnt.prim++;
      const uint4 x_lo = RT_FETCH_LO(pc + RSZ);
      float t;
      if (tri_rec_hit_t(cur_lo, cur_hi, x_lo, o, d, GENB ? t_lo : t_near, best, t)) {
        if (GENB && bmode) {
          best = t;  // boundary query: only the closest t matters
        } else {
#if RT_DEFER_HIT
          hmat = pc | ((cur_hi.w >> 16) & 8u);
          best = t, nhits++;
#else
          hp = vadd(o, smul(t, d)), hmat = cur_hi.z | ((cur_hi.w & F_TEXTURED) << 12);
          if constexpr (SURF) {  // include/rtiow_gpu_surface.h: the shading normal, and (tu, tv) beside hp / hn (the includer's h_tu, h_tv)
            h_tu = 0.f, h_tv = 0.f;
            if (cur_hi.w & F_TRI_ATTR)
              hn = tri_rec_shade(cur_lo, cur_hi, x_lo, RT_FETCH_HI(pc + RSZ), RT_FETCH_LO(pc + 2u * RSZ), RT_FETCH_HI(pc + 2u * RSZ), RT_FETCH_LO(pc + 3u * RSZ),
                                 RT_FETCH_HI(pc + 3u * RSZ), o, d, h_tu, h_tv);
            else hn = tri_rec_normal(cur_hi, x_lo, RT_FETCH_HI(pc + RSZ));
          } else {
            hn = tri_rec_normal(cur_hi, x_lo, RT_FETCH_HI(pc + RSZ));
          }
          best = t, tag = depth, nhits++;
#endif
        }
      }
      pc += (SURF && (cur_hi.w & F_TRI_ATTR)) ? 4u * RSZ : 2u * RSZ;  // (its data record; an attribute triangle's three: flat_scene.h)
    } else if (op == OP_PUSH) {
      const uint32_t kind = (cur_hi.w >> F_KIND_SHIFT) & 7u;
      if (RT_REG_STACK0 && depth == 0u) {  // level 0 rides in registers: every wrapper of the reference's scenes is an outermost one
        sv_o = o, sv_d = d;
      } else {
        float* sp = stack + depth * (6u * 64u) + lane;
        sp[0] = o.x, sp[64] = o.y, sp[128] = o.z, sp[192] = d.x, sp[256] = d.y, sp[320] = d.z;
      }
      depth++;
      const V3 a = mk(u2f(cur_lo.x), u2f(cur_lo.y), u2f(cur_lo.z));
      if (cur_hi.w & F_PRE_TRANSLATE) o = vsub(o, mk(u2f(cur_lo.w), u2f(cur_hi.x), u2f(cur_hi.y)));
      if (kind == XF_TRANSLATE) {
        o = vsub(o, a);
      } else if (kind == XF_ROTATE_Y) {
        o = rot_y(o, -a.x, a.y), d = rot_y(d, -a.x, a.y);
        inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
      } else if (kind == XF_SCALE) {
        o = vdiv(o, a), d = vdiv(d, a);
        inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
      } else if (kind == XF_MOVE) {
        o = vsub(o, smul(time, a));
      }
      pc += RSZ;
    } else if (op == OP_POP) {
      const uint32_t kind = (cur_hi.w >> F_KIND_SHIFT) & 7u;
      depth--;
      if (!RT_DEFER_HIT && hmat != NO_HIT && tag == depth + 1u) {
        const V3 a = mk(u2f(cur_lo.x), u2f(cur_lo.y), u2f(cur_lo.z));
        if (kind == XF_TRANSLATE) {
          hp = vadd(hp, a);
        } else if (kind == XF_ROTATE_Y) {
          hp = rot_y(hp, a.x, a.y), hn = rot_y(hn, a.x, a.y);
        } else if (kind == XF_SCALE) {
          hp = vmul(hp, a), hn = vdiv(hn, a);
        } else if (kind == XF_FLIP) {
          hn = vneg(hn);
        }
        if (cur_hi.w & F_PRE_TRANSLATE) hp = vadd(hp, mk(u2f(cur_lo.w), u2f(cur_hi.x), u2f(cur_hi.y)));
        tag = depth;
      }
      if (RT_REG_STACK0 && depth == 0u) {
        o = sv_o, d = sv_d;
      } else {
        const float* sp = stack + depth * (6u * 64u) + lane;
        o = mk(sp[0], sp[64], sp[128]), d = mk(sp[192], sp[256], sp[320]);
      }
      if (kind == XF_ROTATE_Y || kind == XF_SCALE) inv = mk(1.f / d.x, 1.f / d.y, 1.f / d.z);
      pc += RSZ;
    } else if (op == OP_MEDIUM) {  // ConstantMedium::hit, object.rs:545-575
      if (GENB && (cur_hi.w & F_GENERAL_BOUNDARY)) {
        // enter the boundary's stream for query 1 (object.rs:551): range f32::MIN..f32::MAX; the stream's OP_BEND continues
        bmode = 1u, b_saved = best, best = F32_MAX, t_lo = -F32_MAX;
        pc += RSZ;
      } else {
        const uint4 blo = RT_FETCH_LO(pc + RSZ), bhi = RT_FETCH_HI(pc + RSZ);
        float t1, t2;
        uint32_t n_tests;
        const bool crossed = boundary_pair_t(blo, bhi, o, d, t1, t2, n_tests);
        if (COUNT) cnt.prim += n_tests;
        if (crossed) medium_between(t1, t2, cur_lo, cur_hi, pc, o, d, best, hp, hn, hmat, depth, tag, nhits, root_hits, ev_draws, r_pixel, r_sample, r_event);
        pc = cur_hi.x;  // first record after the boundary's stream
      }
    } else if (op == OP_SEG) {  // in front of the hoisted segment (flat_scene.h)
      // NaN is not ordered: a Rect met with 0 / 0 passes `t < start || t >= end` (object.rs:194-196), so a NaN candidate -- or a NaN
      // `best` from a primitive in front of the segment -- cannot be committed with `<`.  Such a ray steps over this record and
      // executes the segment's records against its own best, as the reference walks them (its tests are then counted twice).
      if (RT_HOIST && load_const(&lc->seg_end) != 0u && !(seg_t != seg_t || best != best)) {
        // the segment's closest candidate (seg_t, seg_pc: hoist_eval, when the ray was created) against what was found before it:
        // `t < t_range.end` of object.rs:99,195 for the one primitive that can still win; its hit record as that primitive builds it
#if RT_DEFER_HIT
        if (seg_t < best) best = seg_t, hmat = seg_pc, nhits++;  // (seg_pc carries the face and the "textured" bit as a hit's pc does)
#else
        if (seg_t < best) {
          const uint32_t w_pc = seg_pc & ~(RSZ - 1u);
          const uint4 w_lo = RT_FETCH_LO(w_pc), w_hi = RT_FETCH_HI(w_pc);
          const uint32_t w_op = w_hi.w & 0xffu;
          if (w_op == OP_SPHERE) {
            const V3 off = mk(u2f(w_lo.x), u2f(w_lo.y), u2f(w_lo.z));
            V3 lo_o = o;
            if (w_hi.w & F_TRANSLATE) lo_o = vsub(o, off);
            if (w_hi.w & F_MOVE) {
              const uint4 mv = RT_FETCH_LO(w_pc + RSZ);
              lo_o = vsub(lo_o, smul(time, mk(u2f(mv.x), u2f(mv.y), u2f(mv.z))));
            }
            V3 p = vadd(lo_o, smul(seg_t, d));
            V3 n = sdiv(p, u2f(w_lo.w));
            if (w_hi.w & F_TRANSLATE) p = vadd(p, off);
            if (w_hi.w & F_FLIP) n = vneg(n);
            hp = p, hn = n;
          } else if (w_op == OP_RECT) {
            const uint32_t axis = (w_hi.w >> F_AXIS_SHIFT) & 3u;
            V3 n = mk(axis == 0 ? 1.f : 0.f, axis == 1 ? 1.f : 0.f, axis == 2 ? 1.f : 0.f);
            if (w_hi.w & F_FLIP) n = vneg(n);
            hp = vadd(o, smul(seg_t, d)), hn = n;
          } else {  // PRISM: the face rides in the low bits of seg_pc
            hp = vadd(o, smul(seg_t, d)), hn = prism_normal(seg_pc & 7u);
          }
          hmat = w_hi.z | ((w_hi.w & F_TEXTURED) << 12);
          best = seg_t, tag = depth, nhits++;
        }
#endif
        pc = cur_hi.z;  // behind the segment's records
      } else {
        pc += RSZ;  // no candidate was evaluated: the records of the segment run like any others
      }
    } else if (GENB && op == OP_BEND) {  // end of a general boundary's stream: `best` < MAX <=> the query hit
      const bool any = best < F32_MAX;
      const uint32_t med_pc = cur_hi.z * RSZ;
      if (any && bmode == 1u) {  // query 2 (object.rs:552): range t1 + 0.0001..f32::MAX over the same stream
        b_t1 = best;
        t_lo = best + 0.0001f, best = F32_MAX, bmode = 2u;
        pc = med_pc + RSZ;
      } else {
        const float t2 = best;
        best = b_saved, t_lo = t_near;
        if (any) {  // both queries hit: object.rs:553-574 with the MEDIUM record's density / material
          const uint4 mlo = RT_FETCH_LO(med_pc), mhi = RT_FETCH_HI(med_pc);
          medium_between(b_t1, t2, mlo, mhi, med_pc, o, d, best, hp, hn, hmat, depth, tag, nhits, root_hits, ev_draws, r_pixel, r_sample, r_event);
        }
        bmode = 0u;
        pc += RSZ;  // MEDIUM.end_pc = the record behind this one
      }
    }
  };

