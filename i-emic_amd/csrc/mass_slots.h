/*
 * mass_slots.h -- where the diagonal mass matrix B meets the Jacobian's coefficient planes: the
 * rows that carry an entry of B and their diagonal slots.  Shared by the two units that shift
 * the assembled Jacobian by a multiple of B: theta.hip (J - B / dt / theta) and eigs.hip
 * (J - sigma B).
 */
#ifndef IEMIC_MASS_SLOTS_H
#define IEMIC_MASS_SLOTS_H

#include "common.h"

namespace iemic {

/* the diagonal slots of the rows with a mass-matrix entry (W and P: B = 0), from the slot table */
constexpr int THETA_ROWS = 4;
constexpr int THETA_VAR[THETA_ROWS] = {UU, VV, TT, SS};
constexpr int THETA_SLOT[THETA_ROWS] = {
    slot_of(UU, pos_of(0, 0, 0), UU), slot_of(VV, pos_of(0, 0, 0), VV),
    slot_of(TT, pos_of(0, 0, 0), TT), slot_of(SS, pos_of(0, 0, 0), SS)};
static_assert(THETA_SLOT[0] == ROW_BEGIN[UU] && THETA_SLOT[1] == ROW_BEGIN[VV] &&
                  THETA_SLOT[2] == ROW_BEGIN[TT] && THETA_SLOT[3] == ROW_BEGIN[SS],
              "every row's first slot is its diagonal");

}  // namespace iemic

#endif
