/* The device scope of bfhip_internal.h (bfDevEnter / bfDevLeave) against recording fakes of the two device-layer calls it is built on:
 * which calls it makes, in which order, and where the fake "current device" stands afterwards.  Stand-alone, no device. */
#include <stdio.h>
#include <string.h>

#include "bfhip_internal.h"

enum { GET = 1, SET = 2 };
static struct { int kind, arg; } calls[16];
static int numCalls, current, failGet, failSet;

int bfdevGetDevice(int *device) {
  calls[numCalls].kind = GET; calls[numCalls++].arg = -1;
  if (failGet) return 3;                 /* the answer is left as it was, like hipGetDevice's */
  *device = current;
  return 0;
}
int bfdevSetDevice(int device) {
  calls[numCalls].kind = SET; calls[numCalls++].arg = device;
  if (failSet) return 7;
  current = device;
  return 0;
}

static int failures;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)
static void reset(int cur) { numCalls = 0; current = cur; failGet = failSet = 0; }
static int isCall(int i, int kind, int arg) { return i < numCalls && calls[i].kind == kind && calls[i].arg == arg; }

int main(void) {
  BfDevScope s;

  /* another device: one query, one set; leave restores */
  reset(0);
  CHECK(bfDevEnter(&s, 2) == 0);
  CHECK(numCalls == 2 && isCall(0, GET, -1) && isCall(1, SET, 2) && current == 2);
  bfDevLeave(&s);
  CHECK(numCalls == 3 && isCall(2, SET, 0) && current == 0);

  /* the same device: the query alone, and nothing to restore */
  reset(1);
  CHECK(bfDevEnter(&s, 1) == 0);
  CHECK(numCalls == 1 && isCall(0, GET, -1));
  bfDevLeave(&s);
  CHECK(numCalls == 1 && current == 1);

  /* -1 keeps the current device: no call at all */
  reset(3);
  CHECK(bfDevEnter(&s, -1) == 0);
  bfDevLeave(&s);
  CHECK(numCalls == 0 && current == 3);

  /* the query fails: the device is set all the same (even to what happens to be current), and never restored */
  reset(0);
  failGet = 1;
  CHECK(bfDevEnter(&s, 0) == 0);
  CHECK(numCalls == 2 && isCall(1, SET, 0));
  bfDevLeave(&s);
  CHECK(numCalls == 2);
  reset(0);
  failGet = 1;
  CHECK(bfDevEnter(&s, 2) == 0);
  CHECK(numCalls == 2 && isCall(1, SET, 2) && current == 2);
  bfDevLeave(&s);
  CHECK(numCalls == 2 && current == 2);

  /* the set fails: its code comes back, the scope is inert */
  reset(0);
  failSet = 1;
  CHECK(bfDevEnter(&s, 2) == 7);
  CHECK(numCalls == 2 && current == 0);
  failSet = 0;
  bfDevLeave(&s);
  CHECK(numCalls == 2 && current == 0);

  /* leave twice: one restore */
  reset(0);
  CHECK(bfDevEnter(&s, 1) == 0);
  bfDevLeave(&s);
  bfDevLeave(&s);
  CHECK(numCalls == 3 && isCall(2, SET, 0) && current == 0);

  /* a zeroed scope (a function that left before it entered): nothing */
  reset(2);
  memset(&s, 0, sizeof s);
  bfDevLeave(&s);
  CHECK(numCalls == 0 && current == 2);

  /* a scope is reusable: the short enter / leave before a second enter of bfhipExtract */
  reset(0);
  CHECK(bfDevEnter(&s, 1) == 0);
  bfDevLeave(&s);
  CHECK(bfDevEnter(&s, 1) == 0);
  CHECK(current == 1);
  bfDevLeave(&s);
  CHECK(numCalls == 6 && current == 0);

  if (failures) return 1;
  printf("device scope clean\n");
  return 0;
}
