// lab/spmv_variants_lab.inc -- LAB ONLY (make lab, -DSTAN_LAB): included inside k_spmv (cg.hip) in front of the product's
// walk over the slots (walk_slots).  VAR 8 is a timing-only kernel (16-B accesses, WRONG results); 14-16 walk a slice's slots in another
// order (tools/placement_map.py).  The product library never compiles this file.
        const int32_t *cp = cols + (int64_t)k0 * 64 + lane;
        const VT *vp = vals + (int64_t)k0 * vstream<VT>::STRIDE + lane;
        if (VAR == 8 && !vstream<VT>::FX && std::is_arithmetic_v<VT>) {  // timing only: 16-B accesses, results are wrong
            typedef std::conditional_t<std::is_arithmetic_v<VT>, VT, float> e2;   // (the 60-bit stream's words are no vector element)
            typedef e2 v2 __attribute__((ext_vector_type(2)));
            const v2 *vq = (const v2 *)(vals + (int64_t)k0 * 9 * 64) + lane;
            for (int32_t k = k0; k + 1 < k1; k += 2) {
                const int64_t c = __builtin_nontemporal_load(cp), c2 = __builtin_nontemporal_load(cp + 64);
                double a[9], b[9];
#pragma unroll
                for (int j = 0; j < 9; j++) { const v2 t = __builtin_nontemporal_load(vq + j * 64); a[j] = (double)t.x; b[j] = (double)t.y; }
                const double x0 = x[3 * c], x1 = x[3 * c + 1], x2 = x[3 * c + 2];
                const double z0 = x[3 * c2], z1 = x[3 * c2 + 1], z2 = x[3 * c2 + 2];
                y0 += a[0] * x0 + a[1] * x1 + a[2] * x2 + b[0] * z0 + b[1] * z1 + b[2] * z2;
                y1 += a[3] * x0 + a[4] * x1 + a[5] * x2 + b[3] * z0 + b[4] * z1 + b[5] * z2;
                y2 += a[6] * x0 + a[7] * x1 + a[8] * x2 + b[6] * z0 + b[7] * z1 + b[8] * z2;
                cp += 128;
                vq += 9 * 64;
            }
        } else if (VAR == 14 || VAR == 15 || VAR == 16) {
            // lab: break the lockstep of neighbouring streams (tools/placement_map.py).  14: odd slices
            // walk their slots back to front; 15: every slice starts at slot (slice % width) and wraps;
            // 16: like 15 with a hashed start.  Same products, other summation order per row.
            const int32_t n = k1 - k0;
            const int32_t rot = VAR == 14 ? 0 : VAR == 15 ? (int32_t)(slice % (n > 0 ? n : 1))
                                                          : (int32_t)(((uint32_t)slice * 2654435761u >> 16) % (uint32_t)(n > 0 ? n : 1));
            const bool rev = VAR == 14 && (slice & 1);
#pragma unroll 2
            for (int32_t i = 0; i < n; i++) {
                int32_t kk = rev ? n - 1 - i : i + rot;
                if (kk >= n) kk -= n;
                const int32_t *cq = cp + (int64_t)kk * 64;
                const VT *vq = vp + (int64_t)kk * vstream<VT>::STRIDE;
                const int64_t c = ld_stream<true>(cq);
                double a[9];
                load9<true, VT>(vq, a);
                double x0 = x[3 * c], x1 = x[3 * c + 1], x2 = x[3 * c + 2];
                if (vstream<VT>::FX) { x0 *= FX48_INV; x1 *= FX48_INV; x2 *= FX48_INV; }
                y0 += a[0] * x0 + a[1] * x1 + a[2] * x2;
                y1 += a[3] * x0 + a[4] * x1 + a[5] * x2;
                y2 += a[6] * x0 + a[7] * x1 + a[8] * x2;
            }
        } else
