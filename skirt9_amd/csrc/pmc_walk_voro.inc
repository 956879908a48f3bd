// pmc_walk_voro.inc -- Voronoi grids (VoronoiMeshSnapshot.cpp:1006-1040, 1058-1188; included by pmc_walk.inc): the cell search and the
// step of a walk, one lane per walk, for the generic walk kernel, the transition / launch kernels and the single rays.  The kernels with
// several lanes per walk on the tables of runs are in pmc_walk_voro_run.inc.
//
// A walk on a Voronoi grid keeps, as its pending segment, the cell w.cell, the exit distance w.ds and -- in w.ci -- the neighbour
// through whose bisecting plane (or the domain wall -1..-6 through which) the path leaves the cell.

    // VoronoiMeshSnapshot::cellIndex: nearest site among the cells listed for the block of the position; -1 outside
    __device__ __forceinline__ int voroCellIndex(const DevScene& S, double x, double y, double z)
    {
        if (!(x >= S.gx0 && x <= S.gx1 && y >= S.gy0 && y <= S.gy1 && z >= S.gz0 && z <= S.gz1)) return -1;
        const int nb = S.vblock_n;
        const int i = max(0, min(nb - 1, (int)(nb * (x - S.gx0) / (S.gx1 - S.gx0))));
        const int j = max(0, min(nb - 1, (int)(nb * (y - S.gy0) / (S.gy1 - S.gy0))));
        const int k = max(0, min(nb - 1, (int)(nb * (z - S.gz0) / (S.gz1 - S.gz0))));
        const int64_t b = ((int64_t)i * nb + j) * nb + k;
        int best = -1;
        double mdist = DBL_MAX;
        const int e = S.vblock_start[b + 1];
        for (int q = S.vblock_start[b]; q < e; ++q)
        {
            const int id = S.vblock_list[q];
            const double2 pxy = *reinterpret_cast<const double2*>(S.vsite + 4 * (int64_t)id);
            const double pz = S.vsite[4 * (int64_t)id + 2];
            const double dx = x - pxy.x, dy = y - pxy.y, dz = z - pz;
            const double idist = dx * dx + dy * dy + dz * dz;
            if (idist < mdist)
            {
                best = id;
                mdist = idist;
            }
        }
        return best;
    }

    // true if site m is certainly the nearest site of the position, i.e. cellIndex would return m: the position is
    // closer to it than to every Voronoi neighbour of m, with a relative margin far above the rounding of the squared
    // distances (a position that close to a face goes through the full search).  Used for the interaction point of a
    // propagation walk, whose cell the walk already knows.
    __device__ __forceinline__ bool voroIsNearest(const DevScene& S, int m, double x, double y, double z)
    {
        if (!(x >= S.gx0 && x <= S.gx1 && y >= S.gy0 && y <= S.gy1 && z >= S.gz0 && z <= S.gz1)) return false;
        const double2 pxy = *reinterpret_cast<const double2*>(S.vsite + 4 * (int64_t)m);
        const double pz = S.vsite[4 * (int64_t)m + 2];
        const double dx = x - pxy.x, dy = y - pxy.y, dz = z - pz;
        const double bound = (dx * dx + dy * dy + dz * dz) * (1. + 1e-9);
        const int e = S.vnbr_start[m + 1];
        bool nearest = true;
        for (int q = S.vnbr_start[m]; q < e; q += 4)
        {
            double d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
            {
                const double* pair = S.vpair + 4 * (int64_t)min(q + j, e - 1);
                const double2 xy = *reinterpret_cast<const double2*>(pair);
                const double2 zi = *reinterpret_cast<const double2*>(pair + 2);
                const double ex = x - xy.x, ey = y - xy.y, ez = z - zi.x;
                const bool site = (q + j < e) && (int)__double_as_longlong(zi.y) >= 0;
                d[j] = site ? ex * ex + ey * ey + ez * ez : DBL_MAX;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!(d[j] > bound)) nearest = false;
        }
        return nearest;
    }

    // the exit of cell m for the position and direction of w (MySegmentGenerator::next, State::Inside, :1088-1150):
    // smallest positive intersection distance with the bisecting planes towards the neighbours and with the domain walls.
    // Returns false (w untouched) if no exit is found.
    // UNROLL neighbours per round (the walk kernel's hot step: 4; the start of a walk in the transition / launch kernels,
    // whose register budget is spent elsewhere: 1)
    // one candidate of the exit search (:1100-1140): neighbour mi (site pix, piy, piz; -1..-6: a domain wall; -7: none)
    __device__ __forceinline__ void voroCandidate(const DevScene& S, double rx, double ry, double rz, double kx, double ky, double kz, double prx,
                                                  double pry, double prz, int mi, double pix, double piy, double piz, double& sq, int& mq)
    {
        double si = 0.;
        if (mi >= 0)
        {
            const double nx = pix - prx, ny = piy - pry, nz = piz - prz;
            const double ndotk = nx * kx + ny * ky + nz * kz;
            if (ndotk > 0)
            {
                const double px = 0.5 * (pix + prx), py = 0.5 * (piy + pry), pz = 0.5 * (piz + prz);
                si = (nx * (px - rx) + ny * (py - ry) + nz * (pz - rz)) / ndotk;
            }
        }
        else if (mi == -1)
            si = (S.gx0 - rx) / kx;
        else if (mi == -2)
            si = (S.gx1 - rx) / kx;
        else if (mi == -3)
            si = (S.gy0 - ry) / ky;
        else if (mi == -4)
            si = (S.gy1 - ry) / ky;
        else if (mi == -5)
            si = (S.gz0 - rz) / kz;
        else if (mi == -6)
            si = (S.gz1 - rz) / kz;
        if (si > 0 && si < sq)
        {
            sq = si;
            mq = mi;
        }
    }

    // the same candidate for the kernels with lane pairs: ONE branch around all six domain walls (a cell at the boundary has one or two of them; the
    // chain of six tests above costs every candidate of every cell six skipped branches)
    __device__ __forceinline__ void voroCandidatePair(const DevScene& S, double rx, double ry, double rz, double kx, double ky, double kz, double prx,
                                                      double pry, double prz, int mi, double pix, double piy, double piz, double& sq, int& mq)
    {
        double si = 0.;
        if (mi >= 0)
        {
            const double nx = pix - prx, ny = piy - pry, nz = piz - prz;
            const double ndotk = nx * kx + ny * ky + nz * kz;
            if (ndotk > 0)
            {
                const double px = 0.5 * (pix + prx), py = 0.5 * (piy + pry), pz = 0.5 * (piz + prz);
                si = (nx * (px - rx) + ny * (py - ry) + nz * (pz - rz)) / ndotk;
            }
        }
        else if (mi > -7)
        {
            // wall -1 .. -6: x0, x1, y0, y1, z0, z1 (:1128-1140): (wall coordinate - position) / direction of its axis
            const int a = -1 - mi;
            const int axis = a >> 1;
            const double lo = axis == 0 ? S.gx0 : axis == 1 ? S.gy0 : S.gz0, hi = axis == 0 ? S.gx1 : axis == 1 ? S.gy1 : S.gz1;
            si = (((a & 1) ? hi : lo) - (axis == 0 ? rx : axis == 1 ? ry : rz)) / (axis == 0 ? kx : axis == 1 ? ky : kz);
        }
        if (si > 0 && si < sq)
        {
            sq = si;
            mq = mi;
        }
    }

    // direction cone of DevScene::vcull: sign pattern (bit a: k_a < 0) * 6 + order of |k_x|, |k_y|, |k_z| (pmc_api.hip `perm`)
    __device__ __forceinline__ int voroCone(double kx, double ky, double kz)
    {
        const int sgn = (kx < 0. ? 1 : 0) | (ky < 0. ? 2 : 0) | (kz < 0. ? 4 : 0);
        const double ax = fabs(kx), ay = fabs(ky), az = fabs(kz);
        int p;
        if (ax >= ay)
            p = ay >= az ? 0 : ax >= az ? 1 : 4;
        else
            p = ax >= az ? 2 : ay >= az ? 3 : 5;
        if (PMC_VORO_CONES == 48) return sgn * 6 + p;
        // the sub-cone: k = a e1 + b e2 + c e3 with x >= y >= z the sorted magnitudes, a = x - y, b = y - z, c = z
        const double x = fmax(ax, fmax(ay, az)), z = fmin(ax, fmin(ay, az)), y = (ax + ay + az) - x - z;
        const double a = x - y, b = y - z, c = z;
        const int sub = a >= b + c ? 0 : b >= a + c ? 1 : c >= a + b ? 2 : 3;
        return (sgn * 6 + p) * 4 + sub;
    }

    template<int UNROLL> __device__ __forceinline__ bool voroEnter(const DevScene& S, Walk& w, int m)
    {
        // the cell's header record: site, density and list bounds in one 64-byte sector
        const double* const heads = S.vhead;
        const double* const pairs = S.vpair;
        const double* head = heads + 8 * (int64_t)m;
        const double2 prxy = *reinterpret_cast<const double2*>(head);
        const double2 przn = *reinterpret_cast<const double2*>(head + 2);
        const int2 bounds = *reinterpret_cast<const int2*>(head + 4);
        const double prx = prxy.x, pry = prxy.y, prz = przn.x;
        const double rx = w.rx, ry = w.ry, rz = w.rz, kx = w.kx, ky = w.ky, kz = w.kz;
        double sq = DBL_MAX;
        const int NO_INDEX = -99;
        int mq = NO_INDEX;
        const int s0 = bounds.x;
        const int e = bounds.y;
        int q = s0;
        if (S.vcull)
        {
            // ---- the first 32 neighbours through the cone's mask: the ones that lie behind the direction are not read.
            // The mask comes in the same round trip as the list bounds; the candidates keep their list order.
            uint32_t keep = ~S.vcull[(int64_t)voroCone(kx, ky, kz) * S.num_cells + m];
            const int cnt = e - s0;
            if (cnt < 32) keep &= (1u << cnt) - 1u;
            // rounds of PMC_VORO_CULL_ROUND neighbours whose gathers are in flight together (written out here: as a function
            // with the mask and the running minimum by reference the kernel got scratch memory and ran 30 % slower)
            while (keep != 0u)
            {
                constexpr int N = UNROLL > 1 ? PMC_VORO_CULL_ROUND : 1;  // (the transition / launch kernels: one at a time, their registers are spent)
                int mi[N];
                double pix[N], piy[N], piz[N];
                int last = 0;
#pragma unroll
                for (int j = 0; j < N; ++j)
                {
                    // (slots beyond the kept neighbours read the last one again and are ignored)
                    const bool have = keep != 0u;
                    if (have)
                    {
                        last = __ffs((int)keep) - 1;
                        keep &= keep - 1u;
                    }
                    const double* pair = pairs + 4 * (int64_t)(s0 + last);
                    const double2 xy = *reinterpret_cast<const double2*>(pair);
                    const double2 zi = *reinterpret_cast<const double2*>(pair + 2);
                    pix[j] = xy.x, piy[j] = xy.y, piz[j] = zi.x;
                    mi[j] = have ? (int)__double_as_longlong(zi.y) : -7;
                }
#pragma unroll
                for (int j = 0; j < N; ++j) voroCandidate(S, rx, ry, rz, kx, ky, kz, prx, pry, prz, mi[j], pix[j], piy[j], piz[j], sq, mq);
            }
            q = s0 + 32;  // (a cell with more neighbours -- two in 10^5 cells of a 10^6-site grid: the rest without a mask)
        }
        // UNROLL neighbours per round: their records of the pair table (site and index in one entry) are gathered
        // together, so that the loads of a round are in flight at once; the candidates are compared in list order
        for (; q < e; q += UNROLL)
        {
            int mi[UNROLL];
            double pix[UNROLL], piy[UNROLL], piz[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j)
            {
                // (entries beyond the list read the last one and are ignored)
                const double* pair = pairs + 4 * (int64_t)min(q + j, e - 1);
                const double2 xy = *reinterpret_cast<const double2*>(pair);
                const double2 zi = *reinterpret_cast<const double2*>(pair + 2);
                pix[j] = xy.x, piy[j] = xy.y, piz[j] = zi.x;
                mi[j] = (q + j < e) ? (int)__double_as_longlong(zi.y) : -7;  // -7: no neighbour
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) voroCandidate(S, rx, ry, rz, kx, ky, kz, prx, pry, prz, mi[j], pix[j], piy[j], piz[j], sq, mq);
        }
        if (mq == NO_INDEX) return false;
        w.cell = m;
        w.ds = sq;
        w.ci = mq;
        w.cj = -1;  // (the next cell's run in an observer's table: not known from here, voroAdvance)
        w.dens = przn.y;
        return true;
    }

    // The same for a peel-off walk towards the observer with table `tab` (DevScene::vobs_run): the cell's header and its kept entries are one run
    // of memory that starts at unit `run`; header and the first FIRST entries are requested together (entries beyond the cell's own are read
    // and ignored: they belong to the next run or the padding), further rounds of FIRST follow only for cells with more.  The winner's entry
    // names the next cell AND its run (w.ci, w.cj).
    template<int FIRST> __device__ __forceinline__ bool voroEnterRun(const DevScene& S, Walk& w, int m, uint32_t run, int tab)
    {
        const double* const runs = tab == 0 ? S.vobs_run[0] : tab == 1 ? S.vobs_run[1] : tab == 2 ? S.vobs_run[2] : S.vobs_run[3];
        const double* const rec = runs + 8 * (int64_t)(run & PMC_VORO_RUN_UNIT_MASK);  // (the link's count is for the kernels with lane pairs)
        const double2 prxy = *reinterpret_cast<const double2*>(rec);
        const double2 przn = *reinterpret_cast<const double2*>(rec + 2);
        const int cnt = *reinterpret_cast<const int*>(rec + 4);
        const double prx = prxy.x, pry = prxy.y, prz = przn.x;
        const double rx = w.rx, ry = w.ry, rz = w.rz, kx = w.kx, ky = w.ky, kz = w.kz;
        double sq = DBL_MAX;
        const int NO_INDEX = -99;
        int mq = NO_INDEX;
        uint32_t runq = 0u;
        int q = 0;
        do
        {
            int mi[FIRST];
            uint32_t ri[FIRST];
            double pix[FIRST], piy[FIRST], piz[FIRST];
#pragma unroll
            for (int j = 0; j < FIRST; ++j)
            {
                // (first round: whatever lies behind the header; later rounds: entries beyond the list read the last one and are ignored;
                // entry e: group e / LANES, {x, y} at word e % LANES of the group, {z, tag} LANES words on)
                const int e = q == 0 ? j : min(q + j, cnt - 1);
                const double* pair = rec + 8 + 4 * PMC_VORO_RUN_LANES * (int64_t)(e / PMC_VORO_RUN_LANES) + 2 * (e % PMC_VORO_RUN_LANES);
                const double2 xy = *reinterpret_cast<const double2*>(pair);
                const double2 zi = *reinterpret_cast<const double2*>(pair + 2 * PMC_VORO_RUN_LANES);
                const long long tag = __double_as_longlong(zi.y);
                pix[j] = xy.x, piy[j] = xy.y, piz[j] = zi.x;
                mi[j] = (int)tag;
                ri[j] = (uint32_t)((unsigned long long)tag >> 32);
            }
#pragma unroll
            for (int j = 0; j < FIRST; ++j)
            {
                const int before = mq;
                voroCandidate(S, rx, ry, rz, kx, ky, kz, prx, pry, prz, (q + j < cnt) ? mi[j] : -7, pix[j], piy[j], piz[j], sq, mq);
                if (mq != before) runq = ri[j];
            }
            q += FIRST;
        } while (q < cnt);
        if (mq == NO_INDEX) return false;
        w.cell = m;
        w.ds = sq;
        w.ci = mq;
        w.cj = (int)runq;
        w.dens = przn.y;
        return true;
    }

    // cell of the position of w and its exit; while no exit is found the position moves on by eps (:1153-1164).
    // Returns false when the position leaves the domain that way.
    // known: the cell of the position if the caller has located it already (every walk of a cycle starts at the same
    // position), -2 otherwise
    __device__ __forceinline__ bool voroLocateAndEnter(const DevScene& S, Walk& w, int known = -2)
    {
        int m = known != -2 ? known : voroCellIndex(S, w.rx, w.ry, w.rz);
        while (true)
        {
            if (m < 0) return false;
            if (voroEnter<1>(S, w, m)) return true;
            w.rx += w.kx * S.eps;
            w.ry += w.ky * S.eps;
            w.rz += w.kz * S.eps;
            m = voroCellIndex(S, w.rx, w.ry, w.rz);
        }
    }

    // after the pending segment: propagate to just beyond the exit (:1169) and prepare the next cell's segment
    // RUNS_ONLY: the caller's walks all have a table (the Voronoi peel-off kernel)
    template<bool RUNS_ONLY = false> __device__ __forceinline__ int voroEnterNext(const DevScene& S, Walk& w, int next, int tab = -1)
    {
        if (tab >= 0 || RUNS_ONLY)
        {
            // (w.cj: the run of the next cell, named by the entry the walk left through; -1 in the first visit of a walk, whose task record
            // knows the cell only)
            uint32_t run = (uint32_t)w.cj;
            if (run == 0xFFFFFFFFu)
                run = (tab == 0 ? S.vobs_start[0] : tab == 1 ? S.vobs_start[1] : tab == 2 ? S.vobs_start[2] : S.vobs_start[3])[next];
            return voroEnterRun<PMC_VORO_RUN_FIRST>(S, w, next, run, tab) ? ST_ACTIVE : ST_SLOW;
        }
        return voroEnter<PMC_VORO_UNROLL>(S, w, next) ? ST_ACTIVE : ST_SLOW;
    }
    __device__ __forceinline__ void voroMove(const DevScene& S, Walk& w)
    {
        const double step = w.ds + S.eps;
        w.rx += w.kx * step;
        w.ry += w.ky * step;
        w.rz += w.kz * step;
    }
    template<bool RUNS_ONLY = false> __device__ __forceinline__ int voroAdvance(const DevScene& S, Walk& w, int tab = -1)
    {
        voroMove(S, w);
        const int next = w.ci;
        if (next < 0) return ST_EXIT;
        return voroEnterNext<RUNS_ONLY>(S, w, next, tab);
    }
    // a cell without exit (ST_SLOW): :1153-1164
    __device__ __forceinline__ bool voroStepSlow(const DevScene& S, Walk& w)
    {
        w.rx += w.kx * S.eps;
        w.ry += w.ky * S.eps;
        w.rz += w.kz * S.eps;
        return voroLocateAndEnter(S, w);
    }
