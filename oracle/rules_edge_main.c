/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.  A stand-alone program around oracle/ataxx_rules_oracle.c, meant to be built with
 * -fsanitize=address,undefined (make -C oracle _build/rules_edge_asan) and fed positions on standard input, one per line:
 *
 *     <blockers mask, decimal> <fen rows> <side>
 *
 * For each it generates the moves, adjudicates, makes every move, writes the FEN and the feature rows of every successor
 * and counts perft to depth 2, and prints "<moves> <result> <perft 2> <sum of the successors' stone counts>" for
 * tests/test_rules_reference.py to compare with the cell-list restatement.  No Python is involved in the sanitized run.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ataxx_rules_oracle.h"

int main(void)
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        char *end;
        const unsigned long long mask = strtoull(line, &end, 10);
        orc_pos p;
        if (*end != ' ' || orc_set_fen(&p, end + 1) != 0) {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
        p.blockers |= mask;
        uint16_t moves[ORC_MAX_MOVES];
        int n = 0;
        const int res = orc_result(&p, NULL, NULL);
        n = orc_movegen(&p, moves);
        long stones = 0;
        for (int i = 0; i < n; i++) {
            orc_pos c = p;
            char fen[80], text[8];
            float feat[196];
            int32_t cells[49];
            orc_makemove(&c, moves[i] & 0xFF, moves[i] >> 8);
            orc_fen(&c, fen, (int)sizeof fen);
            orc_move_string(moves[i], text);
            orc_features(&c, feat);
            orc_board_cells(&c, cells);
            if (orc_policy_index(moves[i]) < 0 || orc_policy_index(moves[i]) >= 833)
                return 3;
            stones += __builtin_popcountll(c.pieces[0]) + __builtin_popcountll(c.pieces[1]);
        }
        printf("%d %d %llu %ld\n", n, res, (unsigned long long)orc_perft(&p, 2), stones);
    }
    return 0;
}
