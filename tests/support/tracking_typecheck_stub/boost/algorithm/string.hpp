#pragma once   /* LoopClosing.h includes it; no declaration it reaches uses it */
